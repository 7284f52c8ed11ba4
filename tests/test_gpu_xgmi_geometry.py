"""The xGMI all-reduce kernels (csrc/kernels/xgmi.hip, csrc/runtime/xgmi.cpp) at 2, 3, 4 and
8 ranks and at bucket sizes that leave chunks ragged, empty or one float4 long.

tests/xgmi_geometry_worker.py holds the cases: one reducer per (arena, mode), driven through
the per-call kernel (4 eager rounds bucket by bucket, then 3 all-reduces per graph replay x 2)
and the persistent kernel called directly in both widths (begin(3) / STEP + 1 / gradients /
one xgmi_wait per channel / copy out / end(), eager and as a graph of the three steps replayed
twice behind a fresh begin).  After every all-reduce, on every rank, the whole result arena and
the rank's gradient arena are compared as int32 with the CPU's expectation: the fp32
rank-order sum (xgmi_worker.rank_order_sum) in the buckets, NaN-payload sentinels in the
64-float gaps and the tail; the sum is also held to |got - S| <= (N-1) 2^-24 sum|x_r| in
fp64, and DONE[c] to blocks(c) x steps, error() and first_error() to 0.  Inputs are randn per
rank, doubled (exactly) by a captured kernel from step to step; at N >= 3 the reversed-order
fp32 sum must differ in bits from the rank-order sum in at least 20 % of an arena's elements.

Arenas: fc (1181120, 18880); four (64, 320, 65600, 18880); linear (7872).  Modes: forced
one, forced two, and auto where it mixes them (fc and four at N >= 3; 65600 floats are
262400 B > 256 KiB, so auto takes it two-shot).  The worker asserts describe() against this
table, computed from the formulas of xgmi.cpp / xg_channel written out again in Python
(chunk = round_up(ceil(n / N), 64), nblk = min(64, ceil(chunk / 4 / 256)),
per = ceil(chunk / 4 / nblk) float4, length of rank d = clamp(n - d chunk, 0, chunk)):

          n  N  mode  chunk  nblk   per  floats per rank
         64  *  one      64    1    16  64
         64  2  two      64    1    16  64,0
         64  3  two      64    1    16  64,2x0
         64  4  two      64    1    16  64,3x0
         64  8  two      64    1    16  64,7x0
        320  *  one     320    1    80  320
        320  2  two     192    1    48  192,128
        320  3  two     128    1    32  2x128,64
        320  4  two     128    1    32  2x128,64,0
        320  8  two      64    1    16  5x64,3x0
       7872  *  one    7872    8   246  7872
       7872  2  two    3968    4   248  3968,3904
       7872  3  two    2624    3   219  3x2624
       7872  4  two    1984    2   248  3x1984,1920
       7872  8  two    1024    1   256  7x1024,704
      18880  *  one   18880   19   249  18880
      18880  2  two    9472   10   237  9472,9408
      18880  3  two    6336    7   227  2x6336,6208
      18880  4  two    4736    5   237  3x4736,4672
      18880  8  two    2368    3   198  7x2368,2304
      65600  *  one   65600   64   257  65600
      65600  2  two   32832   33   249  32832,32768
      65600  3  two   21888   22   249  2x21888,21824   (auto)
      65600  4  two   16448   17   242  3x16448,16256   (auto)
      65600  8  two    8256    9   230  7x8256,7808     (auto)
    1181120  *  one 1181120   64  4614  1181120
    1181120  2  two  590592   64  2307  590592,590528
    1181120  3  two  393728   64  1538  2x393728,393664 (auto)
    1181120  4  two  295296   64  1154  3x295296,295232 (auto)
    1181120  8  two  147648   64   577  7x147648,147584 (auto)

Measured on an MI355X from what the kernels left in the result arena, every round of every
call form (bit-equal to the fp32 reference on every rank, so also its figures).  Largest ratio to the fp64 bound per bucket, and the share of
elements on which the reversed order differs:

    N  fc (1181120, 18880)  four (64, 320, 65600, 18880)   linear   order-sensitive
    2  1.000 0.999          0.797 0.998 1.000 1.000        0.997    -
    3  0.988 0.838          0.520 0.710 0.924 0.857        0.933    31.9 / 31.7 / 32.3 %
    4  0.825 0.725          0.366 0.486 0.718 0.738        0.593    43.7 / 44.1 / 43.3 %
    8  0.495 0.377          0.109 0.208 0.477 0.341        0.440    61.7 / 61.6 / 61.6 %

GPU processes per launch: the N ranks plus this pytest process (9 at 8 ranks).  The ranks
build C.XgmiReducer directly from handles gathered over gloo, PDM_XGMI_PROBE=0: no pre-flight
children (they would make 17) and no self-check writing into the arenas.  Wall time of a
launch, processes' start included, this file run on its own: 5.5 s (N = 2), 5.5 s (3),
6.1 s (4), 17.8 s (8, of which 12.9 s in the cases).  Inside the whole suite's run, whose
tail is profiles/xgmi_geometry/gpu_tests_tail.log, the 8-rank test takes 29.2 s.
test_xgmi_optimizer_in_launch_exchange[4] before this file existed, on the same machine:
7.9 s, so the allowance 2 x 7.9 x N / 4 is 7.9 / 11.8 / 15.8 / 31.6 s.  Eight ranks' spinning
grids stay co-resident on one MI355X (8 x 64 workgroups of the persistent kernel, no LDS):
the 8-rank launch meets no device deadline.

What each check is worth, from three mutations of xgmi.hip in scratch builds, at 3 and 4
ranks (none touches a flag, a wait or a deadline):
 1. the sum phase reading the ranks rotated by r, so that it starts from the rank's own copy:
    test_xgmi_geometry_ranks[3] and [4] fail on comparison 1 (about a third of every bucket's
    elements on ranks > 0, last-bit differences, all within the fp64 bound).  The parent's
    test_xgmi_four_ranks_one_gpu notices as well (randn, bit-exact); its in-launch exchange
    test does not run this code.
 2. the two-shot all-gather push leaving out its last destination for odd w: [3] and [4] fail
    on comparison 1, the sentinel still standing in one rank's copy of every odd workgroup's
    slice (buckets with nblk >= 2: 7872 and larger).  The parent's 4-rank tests notice too:
    the transport's start-up self-check refuses the reducer.
 3. hi of the sum phase from c4 instead of len: [3] and [4] fail on comparison 3 ONLY (the
    64 to 192 floats behind a ragged bucket change in the result arena; every bucket element
    stays right).  Not run against the parent's tests, whose arena has no tail for the extra
    reads; from the code they cannot see it, the floats behind the fc bucket being the conv
    bucket's, rewritten by the next kernel on the same stream.
"""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from conftest import REPO, free_port
from xgmi_geometry_worker import ARENAS, LocalCtl, chosen_modes, geometry, run_arena

pytestmark = pytest.mark.gpu

FORMS = ["call eager", "call graph", "stream narrow eager", "stream narrow graph",
         "stream wide eager", "stream wide graph"]


def test_geometry_formulas():
    """The plain-Python geometry the worker holds describe() against, at the figures the
    kernels' own comments and docs/ state."""
    g = geometry(320, 3, "two")
    assert (g["chunk"], g["lens"]) == (128, [128, 128, 64])
    g = geometry(320, 4, "two")
    assert (g["chunk"], g["blocks"], g["per"], g["lens"]) == (128, 1, 32, [128, 128, 64, 0])
    assert geometry(320, 8, "two")["lens"] == [64] * 5 + [0] * 3
    assert geometry(64, 4, "two")["lens"] == [64, 0, 0, 0]
    g = geometry(7872, 4, "one")
    assert (g["mode"], g["blocks"], g["per"]) == ("one-shot", 8, 246)
    g = geometry(65600, 8, "one")
    assert (g["blocks"], g["per"]) == (64, 257)
    assert geometry(65600, 3, "auto")["mode"] == "two-shot"       # 262400 B > 256 KiB
    assert geometry(65600, 2, "auto")["mode"] == "one-shot"       # two ranks: always
    g = geometry(1181120, 8, "auto")
    assert (g["mode"], g["chunk"], g["lens"][-1]) == ("two-shot", 147648, 147584)
    g = geometry(1181120, 3, "auto")
    assert (g["chunk"], g["lens"][-1], g["blocks"]) == (393728, 393664, 64)
    assert geometry(18880, 8, "auto")["mode"] == "one-shot"
    # auto is run where it mixes the modes: never at 2 ranks, not for the small arena
    assert chosen_modes((1181120, 18880), 4) == ("one", "two", "auto")
    assert chosen_modes((64, 320, 65600, 18880), 3) == ("one", "two", "auto")
    assert chosen_modes((64, 320, 65600, 18880), 2) == ("one", "two")
    assert chosen_modes((7872,), 8) == ("one", "two")


def _report(rec, rank=0):
    g = rec["geometry"]
    print(f"rank {rank} {rec['arena']}/{rec['mode']} N={rec['nranks']} {rec['s']:.2f}s "
          f"n={[b['n'] for b in g]} mode={[b['mode'] for b in g]} "
          f"ratio={[round(q, 3) for q in rec['gpu_ratio']]} "
          f"order={[round(q, 3) for q in rec['order_share']]} "
          f"forms={[(f['form'], f['s']) for f in rec['forms']]}")


def _assert_case(rec):
    assert not rec["aborted"], rec["fails"]
    assert rec["fails"] == [], rec["fails"][:8]
    assert [f["form"] for f in rec["forms"]] == FORMS
    assert all(f["ok"] and f["error"] == 0 and f["first_error"] == 0 for f in rec["forms"])
    assert max(rec["ratio"]) <= 1.0, rec["ratio"]              # the fp32 reference's own
    assert max(rec["gpu_ratio"]) <= 1.0, rec["gpu_ratio"]      # what the GPU left, every round
    if rec["nranks"] >= 3:
        assert rec["order_share_all"] >= 0.20, rec["order_share"]


def test_xgmi_single_rank_gapped_arena(gpu):
    """nranks = 1: the four-channel gapped arena through every mode and call form is the
    identity on the buckets and leaves the sentinels alone."""
    from pytorch_distributed_mnist_amd.ops import _ext
    C = _ext.require()
    name, lens = ARENAS[1]
    assert len(lens) == 4
    for mode in ("one", "two", "auto"):
        rec = run_arena(C, gpu, LocalCtl(), name, lens, mode)
        _report(rec)
        _assert_case(rec)
        assert rec["gpu_ratio"] == [0.0] * 4         # the identity


def test_xgmi_constructor_refusals(gpu):
    """Geometry the kernels cannot serve is refused by the constructor, before any launch."""
    from pytorch_distributed_mnist_amd.ops import _ext
    C = _ext.require()
    grads = torch.zeros(1024, device=gpu)

    def refuse(why, bounds, rank=0, nranks=1, mode="auto"):
        with pytest.raises(RuntimeError, match=why):
            C.XgmiReducer(rank, nranks, 0, grads, bounds, 10.0, mode)

    refuse("64-float aligned", [32, 96])              # start not a multiple of 64
    refuse("64-float aligned", [64, 160])             # length not a multiple of 64
    refuse("buckets as", [0, 64, 64, 128, 128, 192, 192, 256, 256, 320])   # five buckets
    refuse("out of range", [960, 1088])               # past the arena
    refuse("ranks, got 9", [0, 64], nranks=9)
    refuse("bad rank", [0, 64], rank=2, nranks=2)
    refuse(r"auto\|one\|two", [0, 64], mode="three")
    x = C.XgmiReducer(0, 1, 0, grads, [0, 64, 64, 128, 128, 192, 192, 1024], 10.0, "two")
    assert x.num_buckets == 4
    x.close()


def _run_geometry(nproc, tmp_path):
    env = dict(os.environ, PDM_SHARE_DEVICE="1", PDM_XGMI_OUT=str(tmp_path), PDM_XGMI_PROBE="0",
               PDM_XGMI_TIMEOUT="10")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
                        "--master-port", str(free_port()),
                        os.path.join(REPO, "tests", "xgmi_geometry_worker.py")],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=180)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = [json.load(open(tmp_path / f"rank{i}.json")) for i in range(nproc)]
    print(f"geometry launch N={nproc}: wall {wall:.1f}s, cases {out[0]['s']:.1f}s")
    return out


@pytest.mark.parametrize("nproc", [2, 3, 4, 8])
def test_xgmi_geometry_ranks(gpu, tmp_path, nproc):
    """Every arena, mode and call form of the worker at N ranks sharing the GPU: bit equality
    with the CPU's fp32 rank-order sum on every rank, the fp64 bound, sentinels outside the
    buckets in both arenas, DONE counts and clean error words."""
    ranks = _run_geometry(nproc, tmp_path)
    want = [(name, mode) for name, lens in ARENAS for mode in chosen_modes(lens, nproc)]
    for rec in ranks[0]["cases"]:
        _report(rec)
    for d in ranks:
        for rec in d["cases"]:
            if rec["fails"]:
                _report(rec, d["rank"])
                print(f"rank {d['rank']}:", *rec["fails"][:12], sep="\n  ")
    for d in ranks:
        assert [(rec["arena"], rec["mode"]) for rec in d["cases"]] == want, d["rank"]
        for rec in d["cases"]:
            assert rec["nranks"] == nproc
            _assert_case(rec)
