#!/usr/bin/env python3
"""A scene's convergence curve as CSV (iteration, sse, psnr_db): ONE render with the convergence metric on
(PtOptions.convergence, include/pt_amd.h) instead of one render and one full readback per point.
usage: tools/convergence_curve.py SCENE.txt [--res WxH] [--spp N] [--arith exact|fma|fast] [--convergence N | --reference FILE.pfm]
                                  [--clean-db X] [--out curve.csv]
The reference frame is the average after iteration N (default 10, the reference's computePSNR) or an averaged-radiance PFM image
(`pt_render --pfm`, e.g. of a 5000-spp render).  Iterations without a value (<= N) have empty sse / psnr fields; "inf" is the
reference's "Inf" (mse <= 1e-12)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosc_4397_pathtracing_raytracing_project_amd import capi  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--res", default="")
    ap.add_argument("--spp", type=int, default=0, help="iterations (default: the scene file's)")
    ap.add_argument("--arith", default="exact", choices=sorted(capi.ARITH))
    ap.add_argument("--convergence", type=int, default=0, help="capture the reference frame at this iteration (default 10)")
    ap.add_argument("--reference", default="", help="averaged-radiance PFM image to compare with instead")
    ap.add_argument("--clean-db", type=float, default=35.0)
    ap.add_argument("--out", default="-")
    a = ap.parse_args()
    if a.convergence and a.reference:
        ap.error("--convergence and --reference exclude each other")
    if a.convergence < 0:
        ap.error("--convergence wants an iteration >= 1")
    res = tuple(int(v) for v in a.res.split("x")) if a.res else None
    scene = capi.Scene(a.scene, res=res)
    w, h = scene.resolution
    spp = a.spp or scene.iterations
    ref = None
    if a.reference:
        ref = capi.load_pfm(a.reference)
        if ref.shape != (h, w, 3):
            ap.error(f"{a.reference} is {ref.shape[1]}x{ref.shape[0]}, the scene {w}x{h}")
    r = capi.Renderer(scene, arith=a.arith, convergence=-1 if ref is not None else (a.convergence or 10))
    try:
        if ref is not None:
            r.set_reference(ref.reshape(-1, 3))
        r.render(1, spp)
        sse = r.convergence(1, spp)
        clean = r.iterations_to_clean(a.clean_db)
    finally:
        r.free()
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    print("iteration,sse,psnr_db", file=out)
    for i, s in enumerate(sse, 1):
        if s < 0:
            print(f"{i},,", file=out)
        else:
            p = capi.psnr_from_sse(float(s), w * h)
            print(f"{i},{s!r},{'inf' if p == capi.FLT_MAX else repr(p)}", file=out)
    if out is not sys.stdout:
        out.close()
    print(f"iterations to clean ({a.clean_db:g} dB): {clean}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
