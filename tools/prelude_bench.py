"""Step-prelude micro-benchmark at the step's shapes: key ranges of 128 rows x 1024 tokens (group 8) and the token order of
4 segments x 32 768 ids (V = 65 536), each HIP entry point against the torch form it replaces — same process, warm, medians.
    python tools/prelude_bench.py [--rows 128] [--ctx 1024] [--group 8] [--segments 4] [--vocab 65536] [--reps 50] [--out FILE]"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnibiote_amd import masks, ops
from omnibiote_amd import train_encoder as TE

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=128); ap.add_argument("--ctx", type=int, default=1024); ap.add_argument("--group", type=int, default=8)
ap.add_argument("--segments", type=int, default=4); ap.add_argument("--vocab", type=int, default=65536); ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default="", help="also append the result lines to this file")
a = ap.parse_args()
dev = "cuda"
host = TE.synthetic_rows(a.rows, a.ctx, a.vocab, np.random.default_rng(0), single_document=False)
np.random.seed(0)
ids = torch.from_numpy(host).to(dev)
masked = TE.mlm_corrupt(ids)[0].reshape(a.segments, -1).contiguous()      # what the step sorts: ~15 % MASK_TOKEN
ws = ops.token_order_workspace(a.segments, masked.shape[1], a.vocab, dev)


def timeit(fn):
    """(device time of one call [us], host + device time per call with the queue drained before and after [us]), medians"""
    for _ in range(5):
        fn()
    dts, wts = [], []
    for _ in range(a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); fn(); e2.record(); e2.synchronize()
        dts.append(e1.elapsed_time(e2) * 1e3)       # the second of two back-to-back calls
        wts.append(e0.elapsed_time(e2) * 1e3 / 2)
    dts.sort(); wts.sort()
    return dts[len(dts) // 2], wts[len(wts) // 2]


def ranges_torch():
    os.environ["OBTE_PRELUDE_HIP"] = "0"
    try:
        return masks.RangeMask.from_tokens(ids, group=a.group).key_ranges
    finally:
        del os.environ["OBTE_PRELUDE_HIP"]


def order_torch():
    return torch.sort(masked, dim=1, stable=True).indices.to(torch.int32)


assert torch.equal(ops.key_ranges_from_tokens(ids, group=a.group), ranges_torch())
assert torch.equal(ops.token_order(masked, a.vocab, ws=ws), order_torch())
lines = []
for name, hip, ref in ((f"key ranges {a.rows} x {a.ctx} group {a.group}", lambda: ops.key_ranges_from_tokens(ids, group=a.group), ranges_torch),
                       (f"token order {a.segments} x {masked.shape[1]} vocab {a.vocab}", lambda: ops.token_order(masked, a.vocab, ws=ws), order_torch)):
    (hd, hw), (rd, rw) = timeit(hip), timeit(ref)
    lines.append(f"{name:42s} HIP {hd:8.1f} us (enqueue to end {hw:8.1f})   torch form {rd:8.1f} us (enqueue to end {rw:8.1f})   x{rd / hd:.1f}")
for l in lines:
    print(l, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
