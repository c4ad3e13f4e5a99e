"""Host-side tests (no GPU) of the weight-streaming product for small M: its symbol table against its companion header, every
argument check of obte_linear_small_m_bf16 that returns before a launch, and the process-wide obte_small_m_max setting."""
import ctypes as C
import os
import re

import pytest

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_linear_small_m_bf16", "obte_small_m_max_set", "obte_small_m_max")
EPI_ROWDOT = 7   # library-internal (csrc/common.h)


def _err():
    return _lib.lib().obte_last_error().decode()


def test_small_m_symbols_have_their_own_table():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_SMALL_M) == NAMES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnibiote_hip_small_m.h")).read()
    assert set(re.findall(r"^(?:int|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == set(NAMES)
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == len(NAMES)      # and nothing else
    for name in NAMES:
        assert name not in _lib.SYMBOLS and name not in _lib.SYMBOLS_ROWS
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS_SMALL_M[name]
        assert fn.restype is res and list(fn.argtypes) == args                                            # bound by lib(), in the same loop
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def _args(M=2, N=48, K=64, a=P, b=P, d=P, aux=None, ak=1, bk=1, epi=_lib.EPI_NONE, alpha=1.0, **over):
    g = _lib.GemmArgs(a, b, d, aux, None, M, N, K, K, K, N, ak, bk, epi, alpha, 0.0, 0, 0)
    for k, v in over.items():
        setattr(g, k, v)
    return g


def _call(**kw):
    g = _args(**kw)
    return _lib.lib().obte_linear_small_m_bf16(C.byref(g), None)


@pytest.mark.parametrize("kw,rc,word", [
    (dict(M=0), EINVAL, "M"), (dict(M=65), EINVAL, "M"),
    (dict(K=96), EINVAL, "K"), (dict(N=12), EINVAL, "N"),
    (dict(lda=68), EINVAL, "lda"), (dict(ldd=40), EINVAL, "small"),
    (dict(ak=0), EUNSUPPORTED, "layout"), (dict(bk=0), EUNSUPPORTED, "layout"),
    (dict(epi=_lib.EPI_GELU), EUNSUPPORTED, "epilogue"), (dict(epi=_lib.EPI_GELU_BWD, aux=P), EUNSUPPORTED, "epilogue"),
    (dict(epi=_lib.EPI_ADD_DROPOUT, aux=P), EUNSUPPORTED, "epilogue"), (dict(epi=_lib.EPI_ACC32), EUNSUPPORTED, "epilogue"),
    (dict(epi=EPI_ROWDOT), EUNSUPPORTED, "epilogue"),
    (dict(epi=_lib.EPI_ROPE_QK), EINVAL, "ROPE_QK"),                                              # no tables
    (dict(epi=_lib.EPI_ROPE_QK, rope_cos=P, rope_sin=P, rope_T=1, rope_head_dim=64, N=64), EINVAL, "ROPE_QK"),   # N is not 3 C
    (dict(epi=_lib.EPI_ADD), EINVAL, "aux"),
    (dict(epi=_lib.EPI_GELU_ACT, alpha=0.5), EINVAL, "alpha"),
    (dict(a=None), EINVAL, "null"), (dict(b=None), EINVAL, "null"), (dict(d=None), EINVAL, "null"),
])
def test_linear_small_m_rejects_before_any_launch(kw, rc, word):
    assert _call(**kw) == rc
    assert _err().startswith("obte_linear_small_m_bf16:") and word in _err(), _err()


def test_linear_small_m_rejects_a_null_descriptor():
    assert _lib.lib().obte_linear_small_m_bf16(None, None) == EINVAL
    assert _err().startswith("obte_linear_small_m_bf16:") and "null" in _err()


def test_small_m_max_setting():
    lib = _lib.lib()
    start = lib.obte_small_m_max()
    assert 0 <= start <= _lib.SMALL_M_MAX_ROWS == 64
    try:
        assert lib.obte_small_m_max_set(17) == start and lib.obte_small_m_max() == 17
        assert lib.obte_small_m_max_set(0) == 17 and lib.obte_small_m_max() == 0
        assert lib.obte_small_m_max_set(64) == 0 and lib.obte_small_m_max() == 64
        for bad in (-1, 65):
            assert lib.obte_small_m_max_set(bad) == EINVAL
            assert _err().startswith("obte_small_m_max_set:"), _err()
            assert lib.obte_small_m_max() == 64                                                    # unchanged by a rejected call
    finally:
        lib.obte_small_m_max_set(start)
    assert lib.obte_small_m_max() == start


def test_small_m_max_context_manager_restores():
    from omnibiote_amd import ops
    lib = _lib.lib()
    start = lib.obte_small_m_max()
    with ops.small_m_max(3):
        assert lib.obte_small_m_max() == 3
        with ops.small_m_max(0):
            assert lib.obte_small_m_max() == 0
        assert lib.obte_small_m_max() == 3
    assert lib.obte_small_m_max() == start
    with pytest.raises(RuntimeError, match="obte_small_m_max_set"):
        with ops.small_m_max(65):
            pass
    assert lib.obte_small_m_max() == start


@pytest.mark.parametrize("value,want", [("0", 0), (None, 64)])
def test_environment_switch_is_applied_when_the_library_loads(value, want):
    """OBTE_SMALL_M=0 starts obte_small_m_max at 0; without it the default stands.  A process of its own: the library
    reads the variable once, as it loads."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "OBTE_SMALL_M"}
    if value is not None:
        env["OBTE_SMALL_M"] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from omnibiote_amd import _lib; print(_lib.lib().obte_small_m_max())"], cwd=root, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == want
