"""Readers of tests/golden/ref_kernels.bin.gz and ref_kernel_images.bin.gz (oracle/ref_kernels_harness.cpp: the reference's
own kernel bodies and camera fix-up, compiled in place), shared by tests/test_ref_kernel_goldens.py (CPU) and
tests/test_gpu_ref_kernels.py.  Data only: nothing here needs the reference at test time."""
import functools
import os

import numpy as np

import golden_io as gio

SCENE_NAMES = ("cornell", "sphere", "ref_twisted", "ref_quirks")  # the harness's scene numbers
CAMERA_FIELDS = ("position", "lookAt", "view", "up", "right", "fov", "pixelLength")

# shade_branch's bit numbers, in the order of the harness's enum
BRANCHES = ("miss_live", "miss_dead", "hit_dead", "emitter", "emitter_reflective", "kill_d4", "pass_d4", "kill_d63", "pass_d63",
            "scatter_d3", "lobe_specular_r03", "lobe_diffuse_r03", "pure_mirror", "rough_mirror", "diffuse_x_gt_y", "diffuse_x_le_y",
            "axis_px", "axis_nx", "axis_py", "axis_ny", "axis_pz", "axis_nz", "neg_zero_normal", "last_bounce_scatters", "zero_colour_in",
            "iter_1", "iter_4194303", "iter_4194304", "iter_2147483647", "idx_last_pixel", "max_exactly_1_pass", "rough_frame_x_gt_y",
            "rough_frame_x_le_y", "idx_above_2_20")


@functools.lru_cache(maxsize=None)
def kernels() -> dict:
    return gio.load("ref_kernels.bin.gz")


@functools.lru_cache(maxsize=None)
def images() -> dict:
    return gio.load("ref_kernel_images.bin.gz")


def scene_paths(directory) -> list:
    """The four scenes in the harness's order; cornell.txt and sphere.txt are written from the package's generators, whose token
    streams equal the reference's files (tests/test_ref_hot_goldens.py holds that)."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    s = os.path.join(gio.GOLDEN, "scenes")
    return [scenes.write_scene(scenes.cornell_scene_text(), os.path.join(str(directory), "cornell.txt")),
            scenes.write_scene(scenes.sphere_scene_text(), os.path.join(str(directory), "sphere.txt")),
            os.path.join(s, "ref_twisted.txt"), os.path.join(s, "ref_quirks.txt")]


SHADE_SCENE = os.path.join(gio.GOLDEN, "scenes", "ref_shade.txt")


def camera_words(cam) -> np.ndarray:
    """An OrcCamera / PtCamera (the same 84 bytes) as the golden's 21 words."""
    return np.frombuffer(bytes(memoryview(cam).cast("B")), np.uint32).copy()


def image_cases() -> list:
    """[(k, scene number, w, h, depth, first iteration, iterations)]"""
    return [(k,) + tuple(int(x) for x in row) for k, row in enumerate(images()["images"])]


IMAGE_IDS = ["cornell-96x64-d8-i1+8", "cornell-61x37-d8-i1+16", "cornell-48x32-d1-i1+4", "cornell-48x32-d2-i1+4", "cornell-48x32-d5-i1+4",
             "cornell-48x32-d20-i1+4", "sphere-48x32-d4-i1+8", "twisted-48x32-d8-i1+8", "quirks-48x32-d8-i1+8", "cornell-48x32-d8-i4194300+8",
             "cornell-48x32-d8-i2147483600+4"]


def psnr(a, b) -> float:
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(1.0 / mse)


def check_stated_tolerance(img_sum, ref_sum, spp, what):
    """The project's stated image tolerance (include/pt_amd.h), flat: every value finite; at most 0.2 % of the
    pixels off by more than 1e-5 in averaged radiance; PSNR >= 45 dB + 10 log10(spp / 8).  Prints the figures first."""
    a, b = img_sum / np.float32(spp), ref_sum / np.float32(spp)
    bad = int((np.abs(a - b).max(axis=1) > 1e-5).sum()) if np.isfinite(a).all() else -1
    db = psnr(a, b)
    print(f"TOLERANCE {what}: {bad} of {len(a)} pixels off by > 1e-5, PSNR {db:.1f} dB")
    assert np.isfinite(a).all(), what
    assert bad <= 0.002 * len(a), (what, bad, len(a))
    assert db >= 45.0 + 10 * np.log10(spp / 8), (what, db)
    return bad, db


def shade_vectors() -> dict:
    """The shade vectors as arrays: inputs, the kernel's outputs, the branch masks."""
    k = kernels()
    i, o, b = k["shade_in"], k["shade_out"], k["shade_branch"]
    f = gio.f32
    mask = b[:, 0].astype(np.uint64) | (b[:, 1].astype(np.uint64) << np.uint64(32))
    return dict(iter=i[:, 0].astype(np.int32), depth=i[:, 1].astype(np.int32), idx=i[:, 2].astype(np.int32), remaining=i[:, 3].astype(np.int32),
                t=f(i[:, 4]), nrm=f(i[:, 5:8]), mat=i[:, 8].astype(np.int32), pt=f(i[:, 9:12]), o=f(i[:, 12:15]), d=f(i[:, 15:18]),
                color=f(i[:, 18:21]), out_o=o[:, 0:3], out_d=o[:, 3:6], out_color=o[:, 6:9], out_remaining=o[:, 9].astype(np.int32),
                out_replayed=o[:, 10:13], mask=mask)


def has(mask: np.ndarray, name: str) -> np.ndarray:
    return ((mask >> np.uint64(BRANCHES.index(name))) & np.uint64(1)).astype(bool)


def soa(a: np.ndarray) -> np.ndarray:
    """[n, 3] rows -> the [3, n] arrays the stage entry points take."""
    return np.ascontiguousarray(np.asarray(a).T)


def hit_of(v: dict, sel) -> dict:
    return dict(t=np.ascontiguousarray(v["t"][sel]), nrm=soa(v["nrm"][sel]), mat=np.ascontiguousarray(v["mat"][sel]), pt=soa(v["pt"][sel]))
