"""Host-side tests (no GPU) of the optional fp32 accumulation of weight gradients: the buffer store, the policy snapshot, the
command-line flag, the layout of the argument structs that grew, and the combinations the train step refuses."""
import ctypes as C
import gc
import os
import pickle
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_is_keyed_by_identity_and_releases_a_buffer_when_its_parameter_dies():
    from omnibiote_amd.model import Fp32GradStore, LnPartialStore
    for cls in (Fp32GradStore, LnPartialStore):     # one keyed-by-identity base, two kinds of buffer
        store = cls()
        p, q = torch.nn.Parameter(torch.zeros(6, 8, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(3, 8, dtype=torch.bfloat16))
        bp, bq = store.get(p), store.get(q)
        assert bp.dtype == torch.float32 and bp.device == p.device
        if cls is Fp32GradStore:
            assert bp.shape == p.shape and bq.shape == q.shape
        else:                                       # per-workgroup partial sums of the weight's elements
            assert bp.numel() % p.numel() == 0 and bq.numel() * p.numel() == bp.numel() * q.numel()
        assert store.get(p) is bp and store.get(q) is bq and len(store) == 2
        assert not hasattr(p, "acc32") and "acc32" not in vars(p) and not [k for k in vars(p) if "32" in k]
        del p
        gc.collect()
        assert len(store) == 1 and store.get(q) is bq
        del q
        gc.collect()
        assert len(store) == 0


def test_a_pickle_of_the_model_holds_no_fp32_buffer():
    from omnibiote_amd.model import Fp32GradStore, OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = 16, 64, 1, 2, 32, 0.0, True
    m = OmniBioTA(c)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    before = pickle.dumps(m)
    store = Fp32GradStore()
    for p in m.parameters():
        store.get(p).fill_(1.0)
    after = pickle.dumps(m)
    assert len(after) == len(before)
    back = pickle.loads(after)
    assert all(t.dtype != torch.float32 for t in back.parameters())
    assert all(not isinstance(v, torch.Tensor) or v.dtype != torch.float32 for mod in back.modules() for v in vars(mod).values())
    assert len(store) == len(list(m.parameters()))


def test_grad_policy_stays_immutable_with_the_new_fields():
    from omnibiote_amd import _lib as L
    from omnibiote_amd.model import Fp32GradStore, GradPolicy, accumulate_grads_inplace, current_grad_policy
    store = Fp32GradStore()
    pol = GradPolicy(False, L.LN_PARTIAL_MORE, None, None, L.ACC32_MORE, store)
    assert pol.acc32_mode == L.ACC32_MORE and pol.acc32_store is store and pol.accumulate is False
    for name in ("acc32_mode", "acc32_store", "accumulate"):
        with pytest.raises(AttributeError):
            setattr(pol, name, 0)
    with pytest.raises(AttributeError):
        pol.something_else = 1
    assert GradPolicy().acc32_mode == 0 and GradPolicy().acc32_store is None
    with pytest.raises(ValueError):
        GradPolicy(True, 0, None, None, L.ACC32_FIRST, store)     # the fp32 sum replaces the bf16 sum in param.grad
    with pytest.raises(ValueError):
        GradPolicy(False, 0, None, None, 7, store)
    assert current_grad_policy().acc32_mode == 0
    with accumulate_grads_inplace(False, L.LN_PARTIAL_FIRST, acc32_mode=L.ACC32_FIRST, acc32_store=store):
        inner = current_grad_policy()
        assert inner.acc32_mode == L.ACC32_FIRST and inner.acc32_store is store and inner.ln_mode == L.LN_PARTIAL_FIRST
    assert current_grad_policy().acc32_mode == 0
    assert (L.ACC32_FIRST, L.ACC32_MORE, L.ACC32_LAST) == (L.LN_PARTIAL_FIRST, L.LN_PARTIAL_MORE, L.LN_PARTIAL_LAST) == (1, 2, 3)


def test_the_flag_is_off_by_default():
    from omnibiote_amd.train_encoder import parse_args
    assert parse_args([]).fp32_grad_accum is False
    assert parse_args(["--fp32_grad_accum"]).fp32_grad_accum is True
    assert parse_args(["--fp32_grad_accum"]).master_weights is False


def test_ctypes_structs_have_the_headers_sizes_and_offsets(tmp_path):
    from omnibiote_amd import _lib as L
    mine = [L.GemmArgs.acc32.offset, L.GemmArgs.acc32_mode.offset, C.sizeof(L.GemmArgs),
            L.BlockDesc.attn_w_acc32.offset, L.BlockDesc.proj_w_acc32.offset, L.BlockDesc.fc_w_acc32.offset, L.BlockDesc.mlp_w_acc32.offset,
            L.BlockDesc.w_acc32_mode.offset, C.sizeof(L.BlockDesc)]
    assert mine == [152, 160, 168, 224, 232, 240, 248, 256, 264]       # the LP64 layout of include/omnibiote_hip.h
    assert L.GemmArgs._fields_[-2:] == [("acc32", C.c_void_p), ("acc32_mode", C.c_int32)]      # appended: no older field moved
    assert [f[0] for f in L.BlockDesc._fields_[-5:]] == ["attn_w_acc32", "proj_w_acc32", "fc_w_acc32", "mlp_w_acc32", "w_acc32_mode"]
    assert L.EPI_ACC32 == 8
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:   # the same numbers from the compiler's own reading of the header
        src = tmp_path / "off.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "omnibiote_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d",'
                       "offsetof(obte_gemm_args,acc32),offsetof(obte_gemm_args,acc32_mode),sizeof(obte_gemm_args),"
                       "offsetof(obte_block_desc,attn_w_acc32),offsetof(obte_block_desc,proj_w_acc32),offsetof(obte_block_desc,fc_w_acc32),"
                       "offsetof(obte_block_desc,mlp_w_acc32),offsetof(obte_block_desc,w_acc32_mode),sizeof(obte_block_desc),"
                       "(int)OBTE_EPI_ACC32,(int)OBTE_ACC32_LAST);return 0;}\n")
        exe = tmp_path / "off"
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
        assert got == mine + [L.EPI_ACC32, L.ACC32_LAST]
    sizes = (C.c_int64 * 8)()
    n = L.lib().obte_struct_sizes(sizes, 8)          # (lib() itself refuses a mismatch at load time)
    assert n == 6 and sizes[0] == C.sizeof(L.GemmArgs) and sizes[4] == C.sizeof(L.BlockDesc)
    for name in ("obte_acc32_add_bf16", "obte_embedding_bwd_acc32"):
        assert hasattr(L.lib(), name)


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 4)


def test_combinations_that_would_sum_in_bf16_unnoticed_are_refused_at_construction(monkeypatch):
    from omnibiote_amd import train_encoder as TE
    from omnibiote_amd.model import OmniBioTAConfig
    m = _Stub()
    mk = lambda model=m, **kw: TE.TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), None, mini_batch_size=2, n_head=1,
                                            grad_accum="fp32", **kw)
    assert mk().grad_accum == "fp32"
    assert TE.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, mini_batch_size=2, n_head=1).grad_accum == "bf16"
    with pytest.raises(ValueError, match="sync_every_micro_step"):
        mk(sync_every_micro_step=True)
    with pytest.raises(ValueError, match="fused_loss_fn"):
        mk(fused_loss_fn=lambda *a: None)
    with pytest.raises(ValueError, match="loss_impl"):
        mk(loss_impl="torch")
    ck = _Stub()
    ck.config = OmniBioTAConfig(checkpoint_freq=2)
    with pytest.raises(ValueError, match="checkpoint_freq"):
        mk(ck)
    ck.config.checkpoint_freq = 0
    mk(ck)
    for var in ("OBTE_NO_INPLACE_ACCUM", "OBTE_NO_LN_PARTIALS"):
        monkeypatch.setenv(var, "1")
        with pytest.raises(ValueError, match=var):
            mk()
        monkeypatch.delenv(var)
    with pytest.raises(ValueError, match="grad_accum"):
        TE.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, mini_batch_size=2, n_head=1, grad_accum="fp64")
    # the default mode refuses none of them
    TE.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, mini_batch_size=2, n_head=1, sync_every_micro_step=True, loss_impl="torch")
