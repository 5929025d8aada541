"""Micro-benchmark of the place score (vslam_place_score_dev): ms per call for Q query entries against N database entries of R descriptor rows,
against (a) the matrix-core issue floor in the form profiles/match_fp4.json uses and (b) the only way the library had of getting the same numbers
before: vslam_feature_matching_pairs_dev with gate = 0 over the same pairs, timed in the same process.  Also the cost of
KeyframePipeline.loop_closures() beside the step's own time.

    python tools/bench_place.py [--queries 1024] [--entries 1024,4096] [--rows 500,1500] [--windows 5] [--out profiles/place.json]

The database holds N entries at frame 0 and Q at frame 1 of one sequence, min_gap = 1: every query is eligible against exactly the N, the Q x Q
pairs among the queries cost nothing.  Descriptors are uniform random bits with a planted share of near rows (synth.random_descriptors).  A figure is
the median of `--windows` timed windows, each a host clock around enough back-to-back calls to last >= 0.2 s, ending in a synchronise; the profiler
is off.  Floor: 32 x 32 blocks x 4 instructions x 32.5 cycles / (1024 SIMDs x 2.4 GHz), blocks = Q x N x ceil(R / 32)^2.  The matcher path: one call
per query and chunk of max_batch database entries (query side = the entries through d_qitem with the identity selection, train side = the query
entry at stride 0), so d_train_best holds every query row's nearest distance; `--matcher-calls` of those calls are timed and scaled to all of them.
Before anything is timed the first queries' scores are compared with the numpy restatement tests/place_ref.py bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import place_ref as P  # noqa: E402
import stereo_visual_slam_amd as pkg  # noqa: E402
from stereo_visual_slam_amd import synth  # noqa: E402


def timed(call, sync, windows):
    """median ms per call over `windows` windows of >= 0.2 s (the calls per window come from one synchronised call)"""
    call(); sync()
    t0 = time.perf_counter(); call(); sync()
    n = max(3, int(0.2 / max(time.perf_counter() - t0, 1e-6)) + 1)
    wins = []
    for _ in range(windows):
        sync(); t0 = time.perf_counter()
        for _ in range(n):
            call()
        sync()
        wins.append((time.perf_counter() - t0) * 1e3 / n)
    return float(np.median(wins)), [round(x, 4) for x in wins], n


def floor_ms(Q, N, R):
    blocks = Q * N * ((R + 31) // 32) ** 2
    return blocks * 4 * 32.5 / (1024 * 2.4e9) * 1e3


def score_case(vo, Q, N, R, windows, matcher_calls, tau=30):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(R + N)
    # 64 distinct blocks tiled over the entries (the kernel's time does not depend on the bits; the check below does not either)
    blocks = np.stack([synth.random_descriptors(R, R, seed=int(rng.integers(1 << 30)))[k & 1] for k in range(64)])
    total = N + Q
    db = vo.place_db(rows=R, capacity=total, with_geometry=False)
    try:
        d_blocks = torch.from_numpy(blocks).to(dev)
        step = 256
        for e0 in range(0, total, step):
            B = min(step, total - e0)
            idx = (torch.arange(e0, e0 + B, device=dev) * 7) % 64
            d = d_blocks[idx].contiguous()
            n = torch.full((B,), R, dtype=torch.int32, device=dev); seq = torch.zeros(B, dtype=torch.int32, device=dev)
            frame = (torch.arange(e0, e0 + B, device=dev) >= N).to(torch.int32)
            torch.cuda.synchronize()
            vo.place_add_dev(db, d.data_ptr(), R * 32, n.data_ptr(), None, seq.data_ptr(), frame.data_ptr(), None, None, None, 0, B)
        d_score = torch.empty((Q, total), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call = lambda: vo.place_score_dev(db, N, Q, tau, 1, d_score.data_ptr(), total)
        call(); vo.sync()
        got = d_score[:2, :6].cpu().numpy()
        for i in range(2):
            for j in range(6):
                assert got[i, j] == P.score_pair(blocks[((N + i) * 7) % 64], blocks[(j * 7) % 64], tau), ("score check", i, j)
        assert (d_score[:, N:] == -1).all().item() and (d_score[:, :N] >= 0).all().item()
        ms, wins, n_calls = timed(call, vo.sync, windows)
        fl = floor_ms(Q, N, R)
        res = dict(Q=Q, N=N, rows=R, tau=tau, score_ms=round(ms, 4), windows_ms=wins, calls_per_window=n_calls, floor_ms=round(fl, 4),
                   fraction_of_floor=round(fl / ms, 4))
        # the matcher path on the same pairs: per query, chunks of max_batch database entries
        mb = int(vo.params.max_batch)
        n_mb = min(mb, N)
        desc_ptr_holder = torch.zeros((total, (R + 31) // 32 * 32, 32), dtype=torch.uint8, device=dev)   # the same blocks in a caller's buffer
        for e0 in range(0, total, step):
            B = min(step, total - e0)
            idx = (torch.arange(e0, e0 + B, device=dev) * 7) % 64
            desc_ptr_holder[e0:e0 + B, :R] = d_blocks[idx]
        stride = desc_ptr_holder.shape[1] * 32
        d_n = torch.full((total,), R, dtype=torch.int32, device=dev)
        d_sel = torch.arange(R, dtype=torch.int32, device=dev).repeat(total, 1).contiguous()
        d_gap = torch.ones(n_mb, dtype=torch.float64, device=dev)
        d_out = torch.zeros((n_mb, R, 16), dtype=torch.uint8, device=dev); d_nout = torch.zeros(n_mb, dtype=torch.int32, device=dev)
        chunks = [(i, j0) for i in range(Q) for j0 in range(0, N, n_mb)]
        sample = chunks[:: max(1, len(chunks) // matcher_calls)][:matcher_calls]
        qitems = {j0: torch.arange(j0, min(j0 + n_mb, N), dtype=torch.int32, device=dev) for j0 in sorted({c[1] for c in sample})}
        torch.cuda.synchronize()

        def matcher():
            for i, j0 in sample:
                qi = qitems[j0]
                vo.feature_matching_pairs_dev(desc_ptr_holder.data_ptr(), stride, d_n.data_ptr(), d_sel.data_ptr(), d_n.data_ptr(), R, qi.data_ptr(), total,
                                              desc_ptr_holder[N + i].data_ptr(), 0, d_n.data_ptr(), d_gap.data_ptr(), 0, len(qi), R, d_out.data_ptr(), R,
                                              d_nout.data_ptr())
        mms, mwins, _ = timed(matcher, vo.sync, windows)
        scale = len(chunks) / len(sample)
        res.update(matcher_ms=round(mms * scale, 3), matcher_calls_timed=len(sample), matcher_calls_total=len(chunks), matcher_chunk=n_mb,
                   matcher_fraction_of_floor=round(fl / (mms * scale), 4), speedup_over_matcher=round(mms * scale / ms, 3))
        return res
    finally:
        db.close()


def pipeline_case(B, windows):
    """loop_closures() per step beside the step's own time: the default ping-pong batch (every frame past the turn has its twin in the batch)"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(B, anms_num=500, unique_frames=min(64, B), seed=0, ba_windows="tracks", depth="sgbm", render_workers=8)
    try:
        step_ms, _, _ = timed(p.step, p.vo.sync, windows)
        db = p.vo.place_db(rows=500, capacity=B)
        edges = [None]

        def lc():
            db.clear()
            edges[0] = p.loop_closures(db, min_gap=10, min_score=60, K=3)
        lc_ms, wins, _ = timed(lc, p.vo.sync, windows)
        e = edges[0]
        return dict(B=B, step_ms=round(step_ms, 3), loop_closures_ms=round(lc_ms, 3), windows_ms=wins, edges=int(len(e)), accepted=int(e["accepted"].sum()),
                    min_gap=10, min_score=60, K=3)
    finally:
        p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--entries", default="1024,4096")
    ap.add_argument("--rows", default="500,1500")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--matcher-calls", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--pipeline-batch", type=int, default=256, help="0: skip the loop_closures() measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_place: no GPU visible (there is nothing to measure without one)")
    res = dict(windows=a.windows, device=torch.cuda.get_device_name(0), floor="blocks x 4 x 32.5 cycles / (1024 SIMDs x 2.4 GHz)", cases=[])
    vo = pkg.VO(device=0, max_batch=a.max_batch)
    try:
        for R in [int(r) for r in a.rows.split(",")]:
            for N in [int(n) for n in a.entries.split(",")]:
                c = score_case(vo, a.queries, N, R, a.windows, a.matcher_calls)
                print(json.dumps(c), flush=True)
                res["cases"].append(c)
    finally:
        vo.close()
    if a.pipeline_batch > 0:
        res["pipeline"] = pipeline_case(a.pipeline_batch, a.windows)
        print(json.dumps(res["pipeline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
