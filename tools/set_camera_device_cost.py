#!/usr/bin/env python3
"""How a camera move on a live renderer divides between the camera-dependent tables and re-arming the buffers, with the tables built
on the host (pt_set_camera) and on the device (pt_set_camera_ex, PT_SET_CAMERA_DEVICE_TABLES); profiles/set_camera_device_cost.log
is this tool's output.

  tools/set_camera_device_cost.py [--log FILE] [--steps N]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, exact and fast arithmetic.  Per scene and mode ONE renderer: a first
device-path move to the camera it has (it pays the one-time upload of the camera-independent tables and the workspace's allocation,
and is reported apart), then N orbit steps of 2 pi / 16, every step moved to twice — host path, then away and back on the device path,
or the other way round on odd steps — so that both paths build the same tables in the same process on the same machine, alternating.
Four iterations are rendered after every move.  The figures are PtSetCameraTimes (std::chrono::steady_clock inside the library):
tables_ms, rearm_ms, total_ms.  After every pair the eight device tables are compared byte for byte.  One run, nothing averaged but
the medians at the end; no timing is asserted anywhere."""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.devnull)
ap.add_argument("--steps", type=int, default=6)
args = ap.parse_args()
out = open(args.log, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def copy_of(cam):
    c = capi.PtCamera()
    import ctypes
    ctypes.memmove(ctypes.byref(c), ctypes.byref(cam), ctypes.sizeof(c))
    return c


def move(r, cam, device):
    r.set_camera(cam, device_tables=device)
    t = r.set_camera_times()
    r.render(1, 4)
    r.sync()
    return t


say("# camera moves with host-built and device-built tables, MI355X, 1920 x 1080; PtSetCameraTimes in ms (steady_clock inside the library)")
tmp = tempfile.mkdtemp()
for name, text in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(1920, 1080))),
                   ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text())):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    say(f"\n## {name}")
    for arith in ("exact", "fast"):
        scene = capi.Scene(path)
        r = capi.Renderer(scene, arith=arith)
        st = r.stats()
        say(f"[{arith}] pt_init: grid_cells {st.grid_cells}, tight_leaves {st.tight_leaves}, device MB {st.device_bytes / 2**20:.1f}")
        r.render(1, 4)
        r.sync()
        home = copy_of(scene.camera)
        t = move(r, home, False)
        say(f"[{arith}] warm-up move, host path            tables {t.tables_ms:8.3f}  rearm {t.rearm_ms:8.3f}  total {t.total_ms:8.3f}")
        before = r.stats().device_bytes
        t = move(r, home, True)
        say(f"[{arith}] FIRST device-path move (one-time)  tables {t.tables_ms:8.3f}  rearm {t.rearm_ms:8.3f}  total {t.total_ms:8.3f}   "
            f"(+{(r.stats().device_bytes - before) / 2**20:.2f} MB: the camera-independent tables and the workspace; path {t.path}, fallback {t.fallback})")
        rows = {False: [], True: []}
        prev = home
        for step in range(args.steps):
            cam = copy_of(scene.orbit(np.float32(2 * np.pi / 16), 0.0, 0.0))
            order = (False, True) if step % 2 == 0 else (True, False)
            tables = {}
            for k, device in enumerate(order):
                if k:
                    move(r, prev, device)  # away, so that the second move of the pair rebuilds too
                t = move(r, cam, device)
                tables[device] = r.read_tables()
                rows[device].append(t)
                say(f"[{arith}] step {step + 1} {'device' if device else 'host  '} path                  tables {t.tables_ms:8.3f}  rearm {t.rearm_ms:8.3f}  total {t.total_ms:8.3f}"
                    f"   (path {t.path}, fallback {t.fallback}; grid_cells {r.stats().grid_cells}, tight_leaves {r.stats().tight_leaves})")
            say(f"[{arith}] step {step + 1} tables equal byte for byte: {tables[False] == tables[True]}")
            prev = cam
        for device in (False, True):
            med = [statistics.median(getattr(t, f) for t in rows[device]) for f in ("tables_ms", "rearm_ms", "total_ms")]
            say(f"[{arith}] median of {args.steps} {'device' if device else 'host  '} path             tables {med[0]:8.3f}  rearm {med[1]:8.3f}  total {med[2]:8.3f}"
                f"   (tables are {100 * med[0] / med[2]:.0f} % of a move)")
        r.free()
out.close()
