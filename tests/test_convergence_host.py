"""Host side of the convergence metric (PtOptions.convergence; include/pt_amd.h): the PSNR formula of the reference's
computePSNR (pathtrace.cu:198-200), the option's place in PtOptions, the PFM reader and the command line's refusals.
None of this needs a GPU; the device side is tests/test_gpu_convergence.py."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
FLT_MAX = np.finfo(np.float32).max


def psnr_restated(sse, pixels):
    """computePSNR's last lines in numpy: the division in double, the rest in float32."""
    mse = np.float64(sse) / (np.float64(pixels) * 3.0)
    if mse <= 1e-12:
        return FLT_MAX
    return np.float32(10.0) * np.log10(np.float32(1.0) / np.float32(mse), dtype=np.float32)


def test_psnr_from_sse_matches_the_float32_restatement():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rng = np.random.default_rng(7)
    pixels = 200 * 120
    edge = 1e-12 * pixels * 3.0  # sse at which mse == 1e-12 (up to the rounding of the product)
    cases = [(0.0, pixels), (edge, pixels), (np.nextafter(edge, 0), pixels), (np.nextafter(edge, np.inf), pixels),
             (edge * (1 - 1e-9), pixels), (edge * (1 + 1e-9), pixels), (3e-12, 1), (np.nextafter(3e-12, 0), 1),
             (np.nextafter(3e-12, 1), 1), (3.0, 1), (72000.0 * 3, 72000)]
    cases += [(float(s), int(p)) for s, p in zip(10.0 ** rng.uniform(-5, 6, 300), rng.integers(1, 1 << 22, 300))]
    cases += [(float(s), 1920 * 1080) for s in 10.0 ** rng.uniform(-6, 7, 100)]
    seen_inf = seen_finite = 0
    for sse, px in cases:
        got = np.float32(capi.psnr_from_sse(sse, px))
        want = psnr_restated(sse, px)
        if want == FLT_MAX:
            assert got == FLT_MAX, (sse, px, got)
            seen_inf += 1
        else:
            assert got != FLT_MAX and np.isfinite(got), (sse, px, got)
            # log10f of two libms: within 2 ulp of the result
            assert abs(float(got) - float(want)) <= 2 * float(np.spacing(np.abs(want))), (sse, px, got, want)
            seen_finite += 1
    assert seen_inf >= 4 and seen_finite >= 300
    assert capi.psnr_from_sse(3.0, 1) == 0.0 and capi.psnr_from_sse(3e-3, 1) == np.float32(30.0)


def test_convergence_takes_the_reserved_slot_of_ptoptions():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    assert ctypes.sizeof(capi.PtOptions) == 80
    assert capi.PtOptions.convergence.offset == 60 and capi.PtOptions.convergence.size == 4
    assert not hasattr(capi.PtOptions, "reserved")
    assert [getattr(capi.PtOptions, f).offset for f in ("lds_table_kb", "primary_pieces", "paths_pieces", "paths_min_piece")] == [64, 68, 72, 76]
    assert capi.make_options().convergence == 0 and capi.make_options(convergence=-1).convergence == -1
    assert capi.make_options(convergence=10).convergence == 10


def test_pfm_round_trip_is_bit_exact(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rng = np.random.default_rng(3)
    w, h = 37, 11
    img = (rng.standard_normal((w * h, 3)) * 10.0 ** rng.uniform(-20, 20, (w * h, 1))).astype(np.float32)
    img[0] = [0.0, -0.0, np.float32(1e-42)]  # zeros and a denormal
    path = str(tmp_path / "a.pfm")
    capi.save_pfm(path, img, w, h, 1.0)
    back = capi.load_pfm(path)
    assert back.shape == (h, w, 3)
    assert np.array_equal(back.reshape(-1, 3).view(np.uint32), img.view(np.uint32))
    # the division of the writer and the multiplication of the reader: exact for a power of two (normal numbers)
    normal = img.copy()
    normal[0, 2] = 1.5
    capi.save_pfm(path, normal, w, h, 4.0)
    assert np.array_equal(capi.load_pfm(path, samples=4.0).reshape(-1, 3).view(np.uint32), normal.view(np.uint32))
    # a big-endian file (positive scale) reads the same
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n1.0\n" % (w, h))
        f.write(img.reshape(h, w, 3)[::-1].astype(">f4").tobytes())
    assert np.array_equal(capi.load_pfm(path).reshape(-1, 3).view(np.uint32), img.view(np.uint32))
    for bad in (b"P6\n2 2\n-1.0\n" + bytes(48), b"PF\n2 2\n-1.0\n" + bytes(40)):  # wrong magic, truncated
        with open(path, "wb") as f:
            f.write(bad)
        try:
            capi.load_pfm(path)
        except capi.PtError:
            pass
        else:
            raise AssertionError("a broken PFM file was accepted")


def test_pt_render_refuses_contradictory_convergence_flags(scene_dir, tmp_path):
    ref = str(tmp_path / "ref.pfm")
    r = subprocess.run([BIN, scene_dir["cornell"], "--convergence", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "--convergence" in r.stderr
    r = subprocess.run([BIN, scene_dir["cornell"], "--convergence", "10", "--reference", ref], capture_output=True, text=True)
    assert r.returncode == 1 and "exclude" in r.stderr
    r = subprocess.run([BIN, scene_dir["cornell"], "--reference", ref, "--convergence", "10"], capture_output=True, text=True)
    assert r.returncode == 1 and "exclude" in r.stderr
    # a reference image of the wrong size (or none at all) is refused before any device is touched
    r = subprocess.run([BIN, scene_dir["cornell"], "--res", "8x8", "--reference", ref], capture_output=True, text=True)
    assert r.returncode == 1 and "not a PFM image of 8x8" in r.stderr
