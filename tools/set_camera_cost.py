#!/usr/bin/env python3
"""What a camera move on a live renderer (pt_set_camera) costs against a fresh pt_init; profiles/set_camera_cost.log is this
tool's output.

  tools/set_camera_cost.py [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, exact and fast arithmetic.  Per scene and mode: a fresh pt_init (the
first one of the process also pays for the HIP runtime's start), three orbit steps of 2 pi / 16 through pt_set_camera with four
iterations after each, and as the baseline a fresh pt_init at the camera the last step went to, in the same process on the same
machine.  Host wall clock (time.perf_counter around the call through ctypes) next to the library's own PtSetupTimes.  One run, nothing
averaged; no timing is asserted anywhere."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.devnull)
out = open(ap.parse_args().log, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


say("# pt_set_camera against a fresh pt_init, MI355X, 1920 x 1080, exact arithmetic; host wall clock (time.perf_counter around the")
say("# call through ctypes) and PtSetupTimes (std::chrono::steady_clock inside the library); one run, no repetitions averaged")
tmp = tempfile.mkdtemp()
for name, text in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(1920, 1080))),
                   ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text())):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    say(f"\n## {name}")
    t0 = time.perf_counter()
    scene = capi.Scene(path)
    say(f"scene file load                      {ms(t0):9.3f} ms")
    for arith in ("exact", "fast"):
        scene = capi.Scene(path)
        t0 = time.perf_counter()
        r = capi.Renderer(scene, arith=arith)
        wall = ms(t0)
        t = r.setup_times()
        st = r.stats()
        say(f"[{arith}] fresh pt_init                  {wall:9.3f} ms wall   (tables {t.tables_ms:.3f}, upload {t.upload_ms:.3f}, buffers {t.buffers_ms:.3f}, "
            f"probe {t.probe_ms:.3f} ms; grid_cells {st.grid_cells}, tight_leaves {st.tight_leaves}, device MB {st.device_bytes / 2**20:.1f})")
        r.render(1, 4)
        r.sync()
        for step in range(3):
            cam = scene.orbit(np.float32(2 * np.pi / 16), 0.0, 0.0)
            t0 = time.perf_counter()
            r.set_camera(cam)
            wall = ms(t0)
            t = r.setup_times()
            st = r.stats()
            say(f"[{arith}] pt_set_camera, orbit step {step + 1}     {wall:9.3f} ms wall   (set_camera_ms {t.set_camera_ms:.3f}; grid_cells {st.grid_cells}, "
                f"tight_leaves {st.tight_leaves})")
            t0 = time.perf_counter()
            r.render(1, 4)
            r.sync()
            say(f"[{arith}]   4 iterations after it        {ms(t0):9.3f} ms wall")
        r.free()
        t0 = time.perf_counter()
        r = capi.Renderer(scene, arith=arith)  # the baseline: a fresh renderer at the camera the last move went to
        wall = ms(t0)
        t = r.setup_times()
        say(f"[{arith}] fresh pt_init at that camera   {wall:9.3f} ms wall   (tables {t.tables_ms:.3f}, upload {t.upload_ms:.3f}, buffers {t.buffers_ms:.3f}, "
            f"probe {t.probe_ms:.3f} ms)")
        t0 = time.perf_counter()
        r.render(1, 4)
        r.sync()
        say(f"[{arith}]   4 iterations after it        {ms(t0):9.3f} ms wall")
        r.free()
out.close()
