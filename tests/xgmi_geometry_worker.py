"""Geometry cases of the xGMI all-reduce kernels (tests/test_gpu_xgmi_geometry.py).

Launched like tests/xgmi_worker.py (``torch.distributed.run``, PDM_SHARE_DEVICE=1, gloo
control plane, every rank on device 0, one JSON per rank into $PDM_XGMI_OUT), or called
in-process with one rank (``LocalCtl``).  Every rank builds ``C.XgmiReducer`` itself from
the hipIpc handles gathered over gloo: no pre-flight child and no self-check run, so the
GPU processes of a launch are its N ranks, and the result arena holds nothing but what the
cases below put there.

One case = one reducer over a gapped arena (64 floats before, between and behind the
buckets, then a tail of the largest two-shot chunk) in one forced mode, driven through
every call form: the per-call kernel eager and graph-replayed, the persistent kernel in
both widths eager and graph-replayed.  After every all-reduce the whole result arena and
the rank's own gradient arena are compared as int32 with what the CPU expects: the fp32
rank-order sum in the buckets, the sentinels everywhere else.  Nothing here raises on a
wrong number: every rank keeps in step with its peers and the findings go into the JSON.
"""
import json
import os
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import xgmi_worker                                         # noqa: E402
from xgmi_worker import log, rank_order_sum                # noqa: E402

GAP = 64
# (name, bucket lengths in floats); the largest heap first, so later reducers reuse it
ARENAS = (("fc", (1181120, 18880)), ("four", (64, 320, 65600, 18880)), ("linear", (7872,)))
MODES = ("one", "two", "auto")
GRAD_NAN = 0x7FC0BEEF          # gaps of the gradient arena (a quiet NaN with a payload)
RES_NAN = 0x7FC0CAFE           # the result arena before a call form
# csrc/runtime/xgmi.cpp and csrc/xgmi.h, written out again
ONE_SHOT_MAX_BYTES = 256 << 10
STREAM_WG = 64
THREADS = 256
STEPS = 3                      # steps per persistent launch


def _ceil(a, b):
    return -(-a // b)


def geometry(n, nranks, mode):
    """What XgmiReducer derives for a bucket of n floats, and xg_channel's slices of it."""
    two = nranks > 2 and n * 4 > ONE_SHOT_MAX_BYTES
    if mode == "one":
        two = False
    if mode == "two":
        two = nranks > 1
    chunk = _ceil(_ceil(n, nranks), 64) * 64 if two else n
    c4, n4 = chunk // 4, n // 4
    nblk = min(STREAM_WG, max(1, _ceil(c4, THREADS)))
    lens = [4 * min(max(n4 - d * c4, 0), c4) for d in range(nranks)] if two else [n]
    return {"n": n, "mode": "two-shot" if two else "one-shot", "chunk": chunk, "blocks": nblk,
            "per": _ceil(c4, nblk), "lens": lens}


def chosen_modes(lens, nranks):
    """The forced modes, and auto where it picks another mode than both for some bucket."""
    if nranks == 1:
        return MODES
    pick = lambda m: [geometry(n, nranks, m)["mode"] for n in lens]      # noqa: E731
    return tuple(m for m in MODES if m != "auto" or pick(m) not in (pick("one"), pick("two")))


def layout(lens, nranks):
    """Bucket bounds and the arena length: gap | bucket | gap | ... | gap | tail."""
    bounds, off = [], GAP
    for n in lens:
        bounds.append((off, off + n))
        off += n + GAP
    total = off + max(geometry(n, max(nranks, 2), "two")["chunk"] for n in lens)
    for (s, _), n in zip(bounds, lens):         # a whole chunk per rank stays inside the arena
        assert s + nranks * geometry(n, nranks, "two")["chunk"] <= total
    return bounds, total


class DistCtl:
    def __init__(self, rank, ws):
        self.rank, self.ws = rank, ws

    def handles(self, h):
        out = [None] * self.ws
        dist.all_gather_object(out, h)
        return out

    def barrier(self):
        dist.barrier()

    def parts(self, data):
        out = [torch.zeros_like(data) for _ in range(self.ws)]
        dist.all_gather(out, data)
        return out

    def rank_order_sum(self, data):
        return rank_order_sum(data, self.ws)

    def any(self, flag):
        t = torch.tensor([1 if flag else 0], dtype=torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return bool(t.item())


class LocalCtl:
    """One rank, no process group."""
    rank, ws = 0, 1

    def handles(self, h):
        return [h]

    def barrier(self):
        pass

    def parts(self, data):
        return [data.clone()]

    def rank_order_sum(self, data):
        return data.clone()

    def any(self, flag):
        return bool(flag)


def _bits(t):
    return t.view(torch.int32)


def run_arena(C, dev, ctl, name, lens, mode, timeout_s=10.0):
    """One reducer through every call form; returns its record (``fails`` empty: all good,
    ``aborted``: a device wait gave up on some rank and the launch stops here)."""
    rank, ws = ctl.rank, ctl.ws
    t_start = time.perf_counter()
    bounds, total = layout(lens, ws)
    geo = [geometry(n, ws, mode) for n in lens]
    nb = len(lens)
    fails = []
    rec = {"arena": name, "mode": mode, "nranks": ws, "total": total, "geometry": geo,
           "fails": fails, "aborted": False, "forms": []}

    # inputs: randn per rank in the buckets, a NaN payload everywhere else
    gen = torch.Generator().manual_seed(7919 * (rank + 1) + total % 1000)
    mine = torch.full((total,), GRAD_NAN, dtype=torch.int32).view(torch.float32)
    inb = torch.zeros(total, dtype=torch.bool)
    for s, e in bounds:
        mine[s:e] = torch.randn(e - s, generator=gen)
        inb[s:e] = True
    vals = mine[inb]
    cuts = [0]
    for n in lens:
        cuts.append(cuts[-1] + n)

    # the references, from the ranks' inputs alone
    parts = ctl.parts(vals)
    want_vals = ctl.rank_order_sum(vals)
    ref64 = sum(p.double() for p in parts)
    bound64 = (ws - 1) * 2.0 ** -24 * sum(p.abs().double() for p in parts)
    rev = parts[-1].clone()
    for p in reversed(parts[:-1]):
        rev += p
    differs = _bits(rev) != _bits(want_vals)
    rec["order_share"] = [float(differs[a:b].float().mean()) for a, b in zip(cuts, cuts[1:])]
    rec["order_share_all"] = float(differs.float().mean())
    if ws >= 3 and rec["order_share_all"] < 0.20:
        fails.append(f"inputs: the order shows in only {rec['order_share_all']:.1%} of the elements")
    want = torch.full((total,), RES_NAN, dtype=torch.int32).view(torch.float32)
    want[inb] = want_vals

    def ratios(got_vals, sc):
        err = (got_vals.double() - ref64 * sc).abs()
        bnd = bound64 * sc
        q = torch.nan_to_num(err / bnd, nan=float("inf"))      # a NaN result, or 0 / 0
        q[(err == 0) & (bnd == 0)] = 0.0                       # one rank: the sum is the input
        return [float(q[a:b].max()) for a, b in zip(cuts, cuts[1:])]

    rec["ratio"] = ratios(want_vals, 1.0)        # of the fp32 reference itself
    rec["gpu_ratio"] = [0.0] * nb                # of the GPU's results, the largest seen
    if max(rec["ratio"]) > 1.0:
        fails.append(f"reference: fp32 rank-order sum outside the fp64 bound {rec['ratio']}")

    grads = mine.to(dev)
    x = C.XgmiReducer(rank, ws, 0, grads, [b for se in bounds for b in se], timeout_s, mode)
    x.open_peers(ctl.handles(bytes(x.ipc_handle())))
    desc = x.describe()
    for i, (d, g, (s, _)) in enumerate(zip(desc, geo, bounds)):
        got = (int(d["start"]), int(d["n"]), str(d["mode"]), int(d["chunk"]), int(d["blocks"]))
        if got != (s, g["n"], g["mode"], g["chunk"], g["blocks"]) or x.blocks(i) != g["blocks"]:
            fails.append(f"describe: bucket {i} is {got}, the formulas give {g}")
    res = x.result()
    base_dev = mine.to(dev)
    sentinel = torch.full((total,), RES_NAN, dtype=torch.int32).view(torch.float32).to(dev)
    twice = torch.full((1,), 2.0, device=dev)
    views = [grads[s:e] for s, e in bounds]
    sync = x.sync()
    stepw = sync[C.XG_LOC_STEP:C.XG_LOC_STEP + 1]
    state = {"exp": 0, "steps": 0}

    def advance():                       # the step's gradients: the last ones, doubled (exact)
        for v in views:
            v.mul_(twice)

    def new_form():
        """Sentinels back into the result arena (peers store there: between two barriers),
        the gradients back to the inputs."""
        torch.cuda.synchronize()
        ctl.barrier()
        res.copy_(sentinel)
        grads.copy_(base_dev)
        state["exp"] = 0
        torch.cuda.synchronize()
        ctl.barrier()

    def check(tag, got_res, got_grads, exp):
        sc = 2.0 ** exp
        good = True
        expect = want.clone()
        expect[inb] = want_vals * sc
        if not torch.equal(_bits(got_res), _bits(expect)):
            good = False
            bad = _bits(got_res) != _bits(expect)
            for i, (s, e) in enumerate(bounds):
                k = int(bad[s:e].sum())
                if k:
                    j = int(bad[s:e].nonzero()[0])
                    fails.append(f"{tag}: bucket {i} (n={e - s}) {k} wrong, first at {j}: got "
                                 f"{float(got_res[s + j])!r} want {float(expect[s + j])!r}")
            k = int((bad & ~inb).sum())
            if k:
                fails.append(f"{tag}: result arena: {k} sentinels outside the buckets changed, "
                             f"first at {int((bad & ~inb).nonzero()[0])}")
        q = ratios(got_res[inb], sc)                 # of what the GPU left, every time
        rec["gpu_ratio"] = [max(a, b) for a, b in zip(rec["gpu_ratio"], q)]
        if max(q) > 1.0:
            good = False
            fails.append(f"{tag}: ratio to the fp64 bound per bucket {q}")
        if got_grads is not None:
            expect = mine.clone()
            expect[inb] = vals * sc
            if not torch.equal(_bits(got_grads), _bits(expect)):
                good = False
                bad = _bits(got_grads) != _bits(expect)
                fails.append(f"{tag}: gradient arena: {int(bad.sum())} words changed, "
                             f"first at {int(bad.nonzero()[0])}")
        return good

    def form_done(tag, t0, ok, extra=None):
        err, first = int(x.error()), int(x.first_error())
        if err or first:
            fails.append(f"{tag}: error word {err:#x}, first cause {first:#x}")
        f = {"form": tag, "ok": bool(ok), "error": err, "first_error": first,
             "s": round(time.perf_counter() - t0, 3)}
        f.update(extra or {})
        rec["forms"].append(f)
        log(f"{name}/{mode}: {tag} ok={ok} err={err:#x}")
        return ctl.any(err != 0)

    def per_call():
        t0 = time.perf_counter()
        new_form()
        ok = True
        for it in range(4):              # eager: both one-shot stage parities, twice
            advance()
            state["exp"] += 1
            for i in range(nb):
                x.bucket_ready(i)
            x.finalize()
            torch.cuda.synchronize()
            ok = check(f"call eager {it}", res.cpu(), grads.cpu(), state["exp"]) and ok
        if form_done("call eager", t0, ok):
            return True
        t0 = time.perf_counter()
        new_form()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(3):
                advance()
                x.all_ready()
                x.finalize()
        ok = True
        for it in range(2):
            g.replay()
            torch.cuda.synchronize()
            state["exp"] += 3
            ok = check(f"call graph {it}", res.cpu(), grads.cpu(), state["exp"]) and ok
        return form_done("call graph", t0, ok)

    outs = [torch.empty_like(res) for _ in range(STEPS)]

    def pstep(k):
        stepw.add_(1)
        advance()
        for c in range(nb):              # publish READY[c], wait DONE[c]
            C.xgmi_wait(sync, c, [c, x.blocks(c)], timeout_s)
        outs[k].copy_(res)

    def done_words(tag):
        w = sync.cpu()
        steps = int(w[C.XG_LOC_STEP])
        done = [int(w[C.XG_LOC_DONE + c]) for c in range(nb)]
        if steps != state["steps"]:              # begin() keeps the word: it counts them all
            fails.append(f"{tag}: step word {steps} after {state['steps']} steps")
        if done != [x.blocks(c) * steps for c in range(nb)]:
            fails.append(f"{tag}: DONE {done} after {steps} steps of {[x.blocks(c) for c in range(nb)]} blocks")
        return {"steps": steps, "done": done}

    def persistent(wide):
        w = "wide" if wide else "narrow"
        t0 = time.perf_counter()
        new_form()
        x.begin(STEPS, nb, wide)
        for k in range(STEPS):
            pstep(k)
        x.end()
        state["steps"] += STEPS
        torch.cuda.synchronize()
        ok = True
        for k in range(STEPS):
            last = k == STEPS - 1
            ok = check(f"stream {w} eager {k}", outs[k].cpu(), grads.cpu() if last else None,
                       k + 1) and ok
        if form_done(f"stream {w} eager", t0, ok, done_words(f"stream {w} eager")):
            return True
        t0 = time.perf_counter()
        new_form()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for k in range(STEPS):
                pstep(k)
        ok = True
        for it in range(2):
            x.begin(STEPS, nb, wide)
            g.replay()
            x.end()
            state["steps"] += STEPS
            torch.cuda.synchronize()
            for k in range(STEPS):
                last = k == STEPS - 1
                ok = check(f"stream {w} graph {it}.{k}", outs[k].cpu(),
                           grads.cpu() if last else None, STEPS * it + k + 1) and ok
        return form_done(f"stream {w} graph", t0, ok, done_words(f"stream {w} graph"))

    rec["aborted"] = per_call() or persistent(False) or persistent(True)
    torch.cuda.synchronize()
    ctl.barrier()                        # no peer kernel stores here any more
    x.close()
    rec["s"] = round(time.perf_counter() - t_start, 3)
    return rec


def run_all(C, dev, ctl, arenas=ARENAS, timeout_s=10.0):
    out = []
    for name, lens in arenas:
        for mode in chosen_modes(lens, ctl.ws):
            out.append(run_arena(C, dev, ctl, name, lens, mode, timeout_s))
            if out[-1]["aborted"]:       # a device wait gave up: nothing more on this GPU
                return out
    return out


def main():
    rank, ws = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if os.environ.get("PDM_XGMI_LOG_DIR"):
        os.makedirs(os.environ["PDM_XGMI_LOG_DIR"], exist_ok=True)
        xgmi_worker._LOG = open(os.path.join(os.environ["PDM_XGMI_LOG_DIR"], f"rank{rank}.log"), "w")
    torch.set_num_threads(2)             # N ranks share the CPUs as well
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    from pytorch_distributed_mnist_amd.ops import _ext
    C = _ext.require()
    t0 = time.perf_counter()
    cases = run_all(C, dev, DistCtl(rank, ws), timeout_s=float(os.environ.get("PDM_XGMI_TIMEOUT", "10")))
    res = {"rank": rank, "cases": cases, "s": round(time.perf_counter() - t0, 3)}
    with open(os.path.join(os.environ["PDM_XGMI_OUT"], f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
