#!/usr/bin/env python
"""Time link_regions, region_identities, relabel_regions and track_regions (pwcnet_amd/region_tracks.py) at 8 x 448 x 1024 with
256 table rows on two inputs: a scene of two rectangles on a translating background behind moving_regions (two regions an image,
the common case) and label_regions' labels of Bernoulli p = 0.6 masks with sub-pixel flows (the ragged case: thousands of
components, 256 in the table, most waves hold many keys).  Device events around windows of calls, warm-up first, the cases
alternating, several repeats; medians with min and max.  Beside it the numpy restatement's vectorised route on the host
(tests/region_links_ref.py) with the transfers a user would pay (labels, areas and flows down, tables up), one pass: context, not a
target.  Also the bytes each launch must move.  Prints one JSON line (and writes it to --out).

    python scripts/bench_region_tracks.py [--shape 8 448 1024] [--repeats 7] [--iters 5] [--out profiles/region_tracks_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def must_move(N, H, W, R, voters):
    """Bytes per launch that cannot be avoided with this launch plan (the votes' atomics and the small tables left out)."""
    npix, table = N * H * W, 4 * N * R * (R + 2)
    b = {"clear": table,                                              # the vote table out
         "vote": npix * 4 + voters * (8 + 4),                        # labels_a in, the flow and the labels_b gather of the voters
         "rows": table, "columns": table - 8 * N * R,                # the table in, once each
         "match": 4 * N * R * 6,                                     # the two bests in, succ and pred out, two areas
         "identities": 4 * N * R * 3, "relabel": npix * (4 + 4)}     # pred in, ids and age out; labels in, out
    b["link_total"] = b["clear"] + b["vote"] + b["rows"] + b["columns"] + b["match"]
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region_tracks.py needs a GPU")
    import pwcnet_amd as P
    from tests import region_links_ref as L
    N, H, W = args.shape
    R = args.rows
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                 # noqa: E731
    scene = up(L.moving_scene(N + 1, H, W, seed=0)[0])
    matrices = P.fit_motion(scene, model="affine", iters=4)[0]
    labels, count, reg = P.moving_regions(scene, matrices, min_area=16, max_regions=R)[:3]
    inputs = {"rectangles": (labels, count, reg["area"], scene)}
    ragged = up(np.random.RandomState(0).uniform(size=(N + 1, H, W)) < 0.6)
    labels, count, reg = P.label_regions(ragged, max_regions=R)
    inputs["bernoulli0.6"] = (labels, count, reg["area"], up(L.subpixel_flows(N + 1, H, W, seed=1)))

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs, info, moved = {}, {}, {}
    for name, (labels, count, area, flows) in inputs.items():
        la, lb, aa, ab = labels[:N].contiguous(), labels[1:].contiguous(), area[:N].contiguous(), area[1:].contiguous()
        fa, cnt = flows[:N], count[:N].contiguous()
        links = P.link_regions(la, lb, fa, aa, ab)
        pred = links["pred"][:N - 1].contiguous()
        ids = P.region_identities(pred, cnt)[0]
        runs[f"{name}_link_regions"] = lambda la=la, lb=lb, fa=fa, aa=aa, ab=ab: P.link_regions(la, lb, fa, aa, ab)
        runs[f"{name}_region_identities"] = lambda pred=pred, cnt=cnt: P.region_identities(pred, cnt)
        runs[f"{name}_relabel_regions"] = lambda la=la, ids=ids: P.relabel_regions(la, ids)
        runs[f"{name}_track_regions"] = lambda la=la, cnt=cnt, aa=aa, fa=fa: P.track_regions(la, cnt, {"area": aa}, fa)
        voters = int(links["votes"][..., 3].sum())
        info[name] = {"regions_per_image": cnt.cpu().numpy().tolist(), "voters": voters,
                      "links": int((links["succ"] != 0).sum()), "identities": int(ids.max())}
        moved[name] = must_move(N, H, W, R, voters)
    for fn in runs.values():                    # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, args.iters))
    host = {}
    for name, (labels, count, area, flows) in inputs.items():                      # one pass is enough: context
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = [t[:N].cpu().numpy() for t in (labels, count, area, flows)]
        out = L.track_regions(h[0], h[1], h[2], h[3])
        for a in (out[0], out[1], out[2]["succ"], out[2]["pred"]):
            torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        host[f"{name}_track_regions"] = 1e3 * (time.perf_counter() - t0)
    res = {"what": "region tracking, ms per call (device events, medians of alternating windows of calls through the Python API, "
                   "allocations included): <input>_<function>; link_regions on N pairs, region_identities and relabel_regions on N "
                   "images, track_regions on N images (N - 1 links); must_move_bytes = what each launch cannot avoid reading and "
                   "writing; numpy_host_ms = the restatement's track_regions on the host with labels, areas and flows copied down "
                   "and the tables copied up, one pass (context)",
           "shape": args.shape, "rows": R, "repeats": args.repeats, "iters": args.iters,
           "ms": {key: float(np.median(t)) for key, t in ms.items()}, "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "inputs": info, "must_move_bytes": moved, "numpy_host_ms": host,
           "not_measured": "the launches one by one (no profiler run), the votes' atomics, any other shape or row count, R = 1024",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
