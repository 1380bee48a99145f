"""Timing of the index build's encoding step at the bench shape (a GPU-box helper, not a test):
  (1) VectorIndex.encode_rows over the pinned table (MFMA filter + exact refine, csrc/encode_filter.h),
  (2) gpu.encode from the host array (the all-exact kernels; the yardstick),
  (3) index_build._assign + encode_pq in torch (what bench.py builds its tables with; not the reference's arithmetic),
alternated over rounds after a warm-up, in one process; (1) and (2) must give the same bits before anything is timed.
Kernel times come from the handle's own profile records for (1); for (2) run this script under
`rocprofv3 --kernel-trace --stats -- python tools/encode_timing.py --only 2` and read the kernels' totals from its output.
usage: python tools/encode_timing.py [--n 3000000] [--rounds 3] [--only 1|2|3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    import torch
    from freddy_amd import gpu, index_build as ib
    d, m, C = 300, 12, 1000
    x = ib.make_corpus(a.n, seed=3, device="cpu").numpy().astype(np.float32)
    rng = np.random.default_rng(1)
    coarse = x[rng.choice(a.n, C, replace=False)].copy()
    vi = gpu.VectorIndex(np.arange(1, a.n + 1, dtype=np.int32), x)
    for K in (1024, 256):
        cb = np.ascontiguousarray((x[rng.choice(a.n, K, replace=False)] - coarse[rng.integers(0, C, K)][:, :]).reshape(K, m, d // m).transpose(1, 0, 2))
        runs = {1: lambda: vi.encode_rows(cb, coarse=coarse), 2: lambda: gpu.encode(cb, x, coarse=coarse)}

        def torch_path():
            xt, ct, cbt = (torch.from_numpy(v).cuda() for v in (x, coarse, cb))
            cid = ib._assign(xt, ct)
            out = [ib.encode_pq(xt[s:s + (1 << 18)] - ct[cid[s:s + (1 << 18)]], cbt) for s in range(0, a.n, 1 << 18)]
            torch.cuda.synchronize()
            return cid, out
        runs[3] = torch_path
        which = [a.only] if a.only else [1, 2, 3]
        if not a.only:
            r1, r2 = runs[1](), runs[2]()
            assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]), "encode_rows differs from encode"
        for w in which:
            runs[w]()                                   # warm-up
        times = {w: [] for w in which}
        for _ in range(a.rounds):
            for w in which:
                t0 = time.perf_counter()
                runs[w]()
                times[w].append(time.perf_counter() - t0)
        for w in which:
            t = times[w]
            print(f"K={K} path {w}: median {np.median(t) * 1e3:.1f} ms  min {min(t) * 1e3:.1f}  max {max(t) * 1e3:.1f}  (n={a.n})")
        if 1 in which:
            vi.profile_enable()                         # (one more call, with event pairs around its launches)
            runs[1]()
            st, prof = vi.last_encode_stats(), vi.profile_read()
            ms = {k: v[1] for k, v in prof.items()}
            print(f"K={K} encode_rows kernels per call: " + ", ".join(f"{k} {v:.2f} ms" for k, v in sorted(ms.items())))
            up16 = lambda v: (v + 15) // 16 * 16        # dimensions padded to the MFMA k-step
            flops = 3 * 2 * a.n * (m * K * up16(d // m) + C * up16(d))
            if ms.get("encode_filter_kernel"):
                rate = flops / (ms["encode_filter_kernel"] * 1e-3)
                print(f"K={K} filter: {flops / 1e12:.2f} TFLOP f16 MFMA -> {rate / 1e12:.0f} TF/s = {100 * rate / 2.5e15:.1f} % of the 2.5 PF/s f16 peak")
            print(f"K={K} candidates per item {st['candidates'] / st['items']:.3f}, redone {st['redone']}, violations {st['violations']}")
        vi.profile_enable(False)
        if not a.only and K == 256:                     # where it pays least: few rows (the image build and the stage synchronisations stay)
            for n in (1, 64, 4096, 65536):
                t = {1: [], 2: []}
                for r in range(a.rounds + 1):
                    for w, f in ((1, lambda: vi.encode_rows(cb, coarse=coarse, n_rows=n)), (2, lambda: gpu.encode(cb, x[:n], coarse=coarse))):
                        t0 = time.perf_counter()
                        f()
                        if r:
                            t[w].append(time.perf_counter() - t0)
                print(f"K={K} n={n}: encode_rows median {np.median(t[1]) * 1e3:.2f} ms, encode {np.median(t[2]) * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
