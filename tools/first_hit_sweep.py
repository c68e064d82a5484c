#!/usr/bin/env python3
"""Sweep of k_primary's shared form (one trace per chunk and run of iterations): primary_share x primary_pieces on cornell
1920x1080, fast build, on the whole frame and on the row-interleaved tile of rank 0 of N — Msamples/s of 2000 steps, best of
three, beside the per-iteration form (debug_flags 128) and the library's automatic choice.  The automatic values in
csrc/pt_sched.h (auto_shared_pieces) and pt_api.cpp (primary_share_of) come from this table (profiles/first_hit_sharing.log, section 2b).
usage: tools/first_hit_sweep.py [worlds, e.g. 1,8] [shares, e.g. 4,8,13,25,64] [pieces, e.g. 1,2,4,8] [steps]"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosc_4397_pathtracing_raytracing_project_amd import capi, parallel, scenes  # noqa: E402

W, H = 1920, 1080


def arg(i, default):
    return [int(x) for x in (sys.argv[i] if len(sys.argv) > i else default).split(",")]


def rate(sc, topt, steps, **kw):
    r = capi.Renderer(sc, arith="fast", time_kernels=True, **topt, **kw)
    try:
        r.render(1, 200)
        r.sync()
        best = 1e9
        r.reset_stats()
        for _ in range(3):
            r.clear()
            r.sync()
            t0 = time.perf_counter()
            r.render(1, steps)
            r.sync()
            best = min(best, time.perf_counter() - t0)
        st = r.stats()
        return topt["pixel_count"] * steps / best / 1e6, st.intersect_ms / max(1, st.intersect_launches) * 1e3, st.iters_per_batch
    finally:
        r.free()


def main():
    worlds, shares, pieces, steps = arg(1, "1,8"), arg(2, "4,8,13,25,64"), arg(3, "1,2,4,8"), arg(4, "2000")[0]
    path = scenes.write_scene(scenes.cornell_scene_text(res=(W, H)), os.path.join(tempfile.mkdtemp(), "c.txt"))
    sc = capi.Scene(path, res=(W, H))
    for world in worlds:
        topt = parallel.striped_tile_for_rank(W, H, 0, world) if world > 1 else dict(pixel_begin=0, pixel_count=W * H)
        for name, kw in (("per-iteration (debug_flags 128)", dict(debug_flags=128)), ("automatic", {})):
            v, us, k = rate(sc, topt, steps, **kw)
            print(f"world {world} tile {topt['pixel_count']} px K={k:3d} {name:32s} {v:9.1f} Msamples/s  k_paths {us:7.1f} us/launch", flush=True)
        print(f"world {world}: Msamples/s, rows primary_share, columns primary_pieces {pieces}", flush=True)
        for share in shares:
            row = [rate(sc, topt, steps, primary_share=share, primary_pieces=p)[0] for p in pieces]
            print(f"  share {share:3d}: " + " ".join(f"{v:9.1f}" for v in row), flush=True)


if __name__ == "__main__":
    main()
