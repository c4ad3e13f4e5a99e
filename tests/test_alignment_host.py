"""Host-side tests (no GPU) of the pointer checks of the training entry points (include/omnibiote_hip.h, conventions: alignment).
Every call carries a fake pointer and a shape, probability or count that the entry point rejects AFTER its pointer checks, so nothing
is ever launched: with aligned pointers the call gets as far as that rejection, as it did before the checks existed; with one
pointer moved off its boundary it returns OBTE_EINVAL and obte_last_error() names the argument."""
import ctypes as C

import pytest

from omnibiote_amd import _lib

EINVAL = -1
P = 4096   # a non-null, aligned "pointer" for calls that must return before they touch it


def _err():
    return _lib.lib().obte_last_error().decode()


def _gemm(entry):
    def call(a=P, b=P, d=P, aux=P, d2=P, rope_cos=None, rope_sin=None, acc32=None, workspace=None):
        g = _lib.GemmArgs(a, b, d, aux, d2, 0, 64, 64, 64, 64, 64, 1, 1, _lib.EPI_NONE, 1.0, 0.0, 0, 0)   # M = 0: "empty problem"
        g.rope_cos, g.rope_sin, g.acc32 = rope_cos, rope_sin, acc32
        lib = _lib.lib()
        if entry == "ws":
            return lib.obte_gemm_bf16_ws(C.byref(g), workspace, 1 << 20, None)
        if entry == "grouped":
            arr = (_lib.GemmArgs * 1)()
            arr[0] = g
            return lib.obte_gemm_grouped_bf16(arr, 1, None)
        return lib.obte_gemm_bf16(C.byref(g), None)
    return call


def _attn_fwd(qkv=P, o=P):
    a = _lib.AttnFwdArgs(qkv, o, P, None, None, 0, 0, 0, 1, 8, 1, 64, 1.0, 2.0, 0, None, None)             # dropout_p = 2
    return _lib.lib().obte_attn_fwd(C.byref(a), None)


def _attn_bwd(qkv=P, o=P, d_o=P, dqkv=P, rope_cos=None, rope_sin=None, ws=None):
    a = _lib.AttnBwdArgs(qkv, o, d_o, P, P, dqkv, rope_cos, rope_sin, None, None, 0, 0, 0, 1, 8, 1, 64, 1.0, 2.0, 0, None, None, ws, 0, None)
    return _lib.lib().obte_attn_bwd(C.byref(a), None)


def _mt(name, fields):
    """two tensors: the first valid, the second with n = 12, which is rejected after the first one's pointers were checked"""
    def call(**ptr):
        t = _lib.MtArgs()
        for i, n in enumerate((64, 12)):
            for f in ("p", "g", "m", "v"):
                getattr(t, f)[i] = ptr.get(f, P) if i == 0 else P
            t.n[i], t.lr[i], t.weight_decay[i], t.step[i] = n, 1e-3, 0.0, 1
        t.count = 2
        lib = _lib.lib()
        if name == "obte_adamw_multi_bf16":
            return lib.obte_adamw_multi_bf16(C.byref(t), 0.9, 0.999, 1e-8, None, None)
        if name == "obte_adamw_multi_bf16_ref":
            return lib.obte_adamw_multi_bf16_ref(C.byref(t), 0.9, 0.999, 1e-8, None, None)
        return getattr(lib, name)(C.byref(t), P, None)
    return call, fields


def _master(**ptr):
    t = _lib.MtMasterArgs()
    for f in ("p", "g", "master", "m", "v"):
        getattr(t, f)[0] = ptr.get(f, P)
    t.n[0], t.lr[0], t.weight_decay[0], t.step[0], t.count = 12, 1e-3, 0.0, 1, 1
    return _lib.lib().obte_adamw_multi_master(C.byref(t), 0.9, 0.999, 1e-8, None, None)


def _plain(name, args, where):
    """a plain-argument entry point: args is the full list, where maps the argument's name to its index"""
    def call(**ptr):
        a = list(args)
        for k, v in ptr.items():
            a[where[k]] = v
        return getattr(_lib.lib(), name)(*a)
    call.base = lambda n: args[where[n]]
    return call, tuple(where)


LN9 = [P] * 9
# entry point -> (call(**pointers), the checked arguments, the alignment in bytes, a word of the rejection an aligned call reaches)
CASES = {
    "obte_layernorm_fwd": (*_plain("obte_layernorm_fwd", [P] * 5 + [4, 12, 1e-5, None], dict(x=0, w=1, y=2)), 16, "cols"),
    "obte_layernorm_bwd": (*_plain("obte_layernorm_bwd", LN9 + [4, 12, None], dict(dy=0, x=1, w=2, dresid=5, dx=6)), 16, "bad shape"),
    "obte_layernorm_bwd_acc": (*_plain("obte_layernorm_bwd_acc", LN9 + [4, 12, 1, None], dict(dy=0, x=1, w=2, dresid=5, dx=6)), 16, "bad shape"),
    "obte_layernorm_bwd_partial": (*_plain("obte_layernorm_bwd_partial", LN9 + [4, 12, _lib.LN_PARTIAL_FIRST, None], dict(dy=0, x=1, w=2, dresid=5, dx=6)), 16,
                                   "bad shape"),
    "obte_layernorm_bwd_dropout": (*_plain("obte_layernorm_bwd_dropout", [P] * 10 + [4, 12, 0, 0, 0.1, 1, 2, None],
                                           dict(dy=0, x=1, w=2, dresid=5, dx=6, dx_dropped=7)), 16, "bad shape"),
    "obte_gemm_bf16": (_gemm("plain"), ("a", "b", "d", "aux", "d2", "rope_cos", "rope_sin", "acc32"), 16, "empty problem"),
    "obte_gemm_bf16_ws": (_gemm("ws"), ("a", "b", "d", "aux", "d2", "rope_cos", "rope_sin", "acc32", "workspace"), 16, "empty problem"),
    "obte_gemm_grouped_bf16": (_gemm("grouped"), ("a", "b", "d", "aux", "acc32"), 16, "empty problem"),
    "obte_attn_fwd": (_attn_fwd, ("qkv", "o"), 16, "dropout p"),
    "obte_attn_bwd": (_attn_bwd, ("qkv", "o", "d_o", "dqkv", "ws"), 16, "dropout p"),
    "obte_attn_bwd (RoPE tables)": (lambda **p: _attn_bwd(**{"rope_cos": P, "rope_sin": P, **p}), ("rope_cos", "rope_sin"), 8, "dropout p"),
    "obte_rope_qk_inplace": (*_plain("obte_rope_qk_inplace", [P, P, P, 1, 8, 1, 12, 0, None], dict(qkv=0, cos_t=1, sin_t=2)), 16, "head_dim"),
    "obte_embedding_fwd": (*_plain("obte_embedding_fwd", [P, P, P, 4, 12, 64, None], dict(wte=1, out=2)), 16, "cols"),
    "obte_embedding_fwd_dropout": (*_plain("obte_embedding_fwd_dropout", [P, P, P, 4, 12, 64, 0.1, 1, None], dict(wte=1, out=2)), 16, "cols"),
    "obte_dropout_bf16": (*_plain("obte_dropout_bf16", [P, P, 12, 12, 0.1, 1, 7, None], {"in": 0, "out": 1}), 16, "multiple of 8"),
    "obte_embedding_bwd": (*_plain("obte_embedding_bwd", [P] * 5 + [4, 12, 64, None], dict(dout=2, dwte=3, ws=4)), 16, "bad shape"),
    "obte_embedding_bwd_acc": (*_plain("obte_embedding_bwd_acc", [P] * 5 + [4, 12, 64, 1, None], dict(dout=2, dwte=3, ws=4)), 16, "bad shape"),
    "obte_embedding_bwd_dropout": (*_plain("obte_embedding_bwd_dropout", [P] * 5 + [4, 12, 64, 0, 0.1, 1, None], dict(dout=2, dwte=3, ws=4)), 16, "bad shape"),
    "obte_embedding_bwd_acc32": (*_plain("obte_embedding_bwd_acc32", [P] * 6 + [4, 12, 64, _lib.ACC32_LAST, 0.0, 0, None], dict(dout=2, acc32=3, dwte=4, ws=5)), 16,
                                 "bad shape"),
    "obte_acc32_add_bf16": (*_plain("obte_acc32_add_bf16", [P, P, P, 12, _lib.ACC32_LAST, None], dict(acc32=0, src=1, out=2)), 16, "multiple of 8"),
    "obte_masked_ce_fwd_bwd": (*_plain("obte_masked_ce_fwd_bwd", [P] * 4 + [1.0] + [P] * 3 + [4, 12, None], dict(logits=0, dlogits=7)), 16, "vocab"),
    "obte_masked_ce_fwd_bwd_reuse": (*_plain("obte_masked_ce_fwd_bwd_reuse", [P] * 5 + [1.0] + [P] * 2 + [4, 12, None], dict(logits=0, dlogits=7)), 16, "vocab"),
    "obte_masked_ce_rows": (*_plain("obte_masked_ce_rows", [P] * 4 + [1.0] + [P, P, 2 * P] + [4, 4, 12, None], dict(logits=0, dlogits_rows=7)), 16, "vocab"),
    "obte_rows_gather_bf16": (*_plain("obte_rows_gather_bf16", [P, P, P, 4, 8, 12, None], dict(src=0, dst=2)), 16, "cols"),
    "obte_rows_scatter_bf16": (*_plain("obte_rows_scatter_bf16", [P, P, P, 4, 8, 12, None], dict(src=0, dst=2)), 16, "cols"),
    "obte_adamw_bf16": (*_plain("obte_adamw_bf16", [P] * 4 + [12, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None], dict(p=0, g=1, m=2, v=3)), 16, "multiple of 8"),
    "obte_sumsq_bf16": (*_plain("obte_sumsq_bf16", [P, 12, P, None], dict(g=0)), 16, "multiple of 8"),
    "obte_adamw_multi_bf16": (*_mt("obte_adamw_multi_bf16", ("p", "g", "m", "v")), 16, "tensor 1"),
    "obte_adamw_multi_bf16_ref": (*_mt("obte_adamw_multi_bf16_ref", ("p", "g", "m", "v")), 16, "tensor 1"),
    "obte_sumsq_multi_bf16": (*_mt("obte_sumsq_multi_bf16", ("g",)), 16, "tensor 1"),
    "obte_sumsq_multi_bf16_each": (*_mt("obte_sumsq_multi_bf16_each", ("g",)), 16, "tensor 1"),
    "obte_sumsq_multi_bf16_partials": (*_mt("obte_sumsq_multi_bf16_partials", ("g",)), 16, "tensor 1"),
    "obte_adamw_multi_master": (_master, ("p", "g", "master", "m", "v"), 16, "multiple of 8"),
    "obte_key_ranges_from_tokens": (*_plain("obte_key_ranges_from_tokens", [P, 0, 8, 3, 0, 0, P, None], dict(ids=0, key_ranges=6)), 8, "bad shape"),
    "obte_causal_bounds": (*_plain("obte_causal_bounds", [P, 0, 8, 2 * P, 3 * P, None], dict(doc_ranges=0, key_ranges=3, query_bounds=4)), 8, "bad shape"),
}


@pytest.mark.parametrize("entry", list(CASES))
def test_aligned_pointers_get_as_far_as_before(entry):
    call, _, _, word = CASES[entry]
    assert call() == EINVAL
    assert word in _err() and "aligned" not in _err(), _err()


@pytest.mark.parametrize("entry", list(CASES))
def test_a_misaligned_pointer_is_refused_by_name(entry):
    call, names, align, _ = CASES[entry]
    who = entry.split(" ")[0]
    who = {"obte_gemm_bf16_ws": "obte_gemm_bf16", "obte_gemm_grouped_bf16": "obte_gemm_bf16", "obte_layernorm_bwd_acc": "obte_layernorm_bwd",
           "obte_layernorm_bwd_partial": "obte_layernorm_bwd", "obte_layernorm_bwd_dropout": "obte_layernorm_bwd", "obte_embedding_fwd_dropout": "obte_embedding_fwd",
           "obte_embedding_bwd_acc": "obte_embedding_bwd", "obte_embedding_bwd_dropout": "obte_embedding_bwd",
           "obte_masked_ce_fwd_bwd_reuse": "obte_masked_ce_fwd_bwd"}.get(who, who)      # the forms that share one implementation report under its name
    for name in names:
        base = getattr(call, "base", lambda n: P)(name)
        for off in (2, align // 2):
            assert call(**{name: base + off}) == EINVAL, (entry, name, off)
            e = _err()
            assert e.startswith(who + ":") and f"{name} must be {align}-byte aligned" in e, (entry, name, off, e)
