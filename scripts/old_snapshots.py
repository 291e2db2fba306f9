"""Config 2 with old snapshots, outside bench.py: the window and the ranges of
bench.py's config 2, the snapshots drawn from the most recent `snap_recent`
fraction of the commits -- 0.01 is bench.py's workload, 1.0 draws them from
the whole window, where the locate's slot filter can drop few join records and
the recent lists rarely answer.

    python scripts/old_snapshots.py [--snap-recent 0.01 1.0] [--batches 6]
                                    [--steps 24] [--regions 5]

Per snap_recent one line: us per batch on one stream and on two (the median of
`regions` timed regions of `steps` probes over a ring of `batches` batches),
the conflict rate, join records per batch and full_tile_joins per batch, and
(a library that has hsc_join_stats) the column batches each join kernel took
and the tiles the wave-per-tile join left to a whole block, over all of the
setting's probes.
HSC_LIB picks the library, as everywhere.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snap-recent", type=float, nargs="+", default=[0.01, 1.0])
    ap.add_argument("--n-commits", type=int, default=1_000_000)
    ap.add_argument("--n-txn", type=int, default=100_000)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--regions", type=int, default=5)
    args = ap.parse_args()

    import torch

    from bench import probe_struct, upload_batch
    from comdb2_amd import hsc
    from comdb2_amd.workloads import SEED_CONFIG2, config2, config2_device_window

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    v = hsc.Validator(0)
    assert v.register_group("t1", 0, 9) == 0
    c2 = config2(seed=SEED_CONFIG2, n_commits=args.n_commits, n_txn=1, build_log=False)
    gid, words, lsn = config2_device_window(c2)
    tg = torch.from_numpy(gid).to(dev)
    tw = torch.from_numpy(words.reshape(-1).view(np.int64)).to(dev)
    tl = torch.from_numpy(lsn.view(np.int64)).to(dev)
    v.ingest_device(len(lsn), words.shape[0], tg.data_ptr(), tw.data_ptr(), tl.data_ptr(), c2.params["end_lsn"])
    del tg, tw, tl
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(device=dev)]
    T = args.n_txn
    verdicts = [torch.zeros(T, dtype=torch.uint8, device=dev) for _ in streams]
    has_join_stats = hasattr(v.lib, "hsc_join_stats")
    for sr in args.snap_recent:
        j0 = v.join_stats() if has_join_stats else None
        batches = []
        for bi in range(args.batches):
            rs = config2(seed=SEED_CONFIG2 + 7919 * bi, n_commits=args.n_commits, n_txn=T,
                         snap_recent=sr, build_log=False).readsets
            batches.append(upload_batch(torch, dev, v.marshal(rs)))
        structs = [[probe_struct(hsc, b, verdicts[si], None, T) for si in range(2)] for b in batches]
        torch.cuda.synchronize()

        def region(nstreams):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                v.set_stream(streams[k % nstreams].cuda_stream)
                v.probe_device(structs[k % len(batches)][k % nstreams])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e6

        out = {}
        for ns in (1, 2):
            region(ns)  # warm-up
            out[ns] = float(np.median([region(ns) for _ in range(args.regions)]))
        v.set_stream(streams[0].cuda_stream)
        # one more pass over the ring with the counters read
        full0 = v.batch_stats()["full_tile_joins"]
        v.enable_timing(True)
        recs, conf = [], []
        for k in range(len(batches)):
            v.probe_device(structs[k][0])
            v.synchronize()
            recs.append(v.timing()["records"])
            conf.append(float((verdicts[0].cpu().numpy() != 0).mean()))
        v.enable_timing(False)
        full = (v.batch_stats()["full_tile_joins"] - full0) / len(batches)
        print(f"snap_recent {sr}: one stream {out[1]:.2f} us/batch, two streams {out[2]:.2f} us/batch, "
              f"conflicts {np.mean(conf):.3f}, join records per batch {int(np.mean(recs))}, "
              f"full_tile_joins per batch {full:.0f}", flush=True)
        if has_join_stats:
            j1 = v.join_stats()
            print("    " + ", ".join(f"{k} +{j1[k] - j0[k]}" for k in j1), flush=True)
    v.close()


if __name__ == "__main__":
    main()
