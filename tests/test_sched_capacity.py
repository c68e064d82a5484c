"""A worker context planned for `capacity` pixels runs any list of m <= capacity pixels (csrc/pt_post.cpp set_worker_live): K, Q and
every buffer stay the capacity's, and nq, seg_cap and cap are planned again from pt_sched.h queue_plan(m, Q, K).  That is sound
because queue_plan is monotone in N for fixed Q and K: every index the smaller plan forms lies inside the larger plan's buffers.
tests/sched_capacity_driver.cpp, built with the system compiler, prints the plan of EVERY m <= capacity; here it is checked by
enumeration, without a GPU."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """[(capacity, Q, K, plans int64 [capacity + 1, 3])]: plans[m] = (nq, seg_cap, cap) of m pixels, row 0 unused."""
    exe = str(tmp_path_factory.mktemp("sched_capacity") / "sched_capacity_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_capacity_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    out = []
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        if line.startswith("case"):
            f = {k: int(v) for k, v in (t.split("=") for t in line.split()[1:])}
            out.append((f["capacity"], f["Q"], f["K"], []))
        else:
            out[-1][3].append([int(v) for v in line.split()])
    full = []
    for capacity, Q, K, changes in out:
        ch = np.array(changes, np.int64)
        assert ch[0, 0] == 1 and np.all(np.diff(ch[:, 0]) > 0) and ch[-1, 0] <= capacity  # from m = 1 on, in order
        runs = np.diff(np.append(ch[:, 0], capacity + 1))
        plans = np.vstack([np.zeros((1, 3), np.int64), np.repeat(ch[:, 1:], runs, axis=0)])
        assert plans.shape == (capacity + 1, 3)
        full.append((capacity, Q, K, plans))
    return full


def test_the_sweep_covers_the_tiles_of_the_gpu_tests_and_a_quarter_of_1080p(cases):
    have = {(c, Q, K) for c, Q, K, _ in cases}
    assert {(1067, 256, 3), (5184, 256, 256), (1296, 256, 256), (1920 * 1080 // 4, 256, 98)} <= have and {Q for _, Q, _ in have} >= {1, 4, 256, 1024}


def test_queue_plan_is_what_the_header_says(cases):
    for capacity, Q, K, plans in cases:
        m = np.arange(1, capacity + 1)
        nq = -(-(-(-m // 64)) // Q)  # ceil(ceil(m / 64) / Q)
        assert np.array_equal(plans[1:, 0], nq) and np.array_equal(plans[1:, 1], 64 * nq) and np.array_equal(plans[1:, 2], K * 64 * nq), (capacity, Q, K)
        assert plans[1:].min() >= 1 and np.all(Q * plans[1:, 1] >= m)  # every pixel has a slot in some queue's region


def test_queue_plan_is_monotone_so_a_live_plan_fits_the_capacity_buffers(cases):
    for capacity, Q, K, plans in cases:
        assert np.all(np.diff(plans[1:], axis=0) >= 0), (capacity, Q, K)  # nq, seg_cap and cap never fall as m grows
        nq_c, seg_c, cap_c = plans[capacity]
        nq, seg, cap = plans[1:, 0], plans[1:, 1], plans[1:, 2]
        # what the buffers are sized with (csrc/pt_api.cpp alloc_batch_buffers): path planes of Q * cap slots, Q * K regions of seg_cap records
        assert np.all(Q * cap <= Q * cap_c) and np.all(Q * K * seg <= Q * K * seg_c) and np.all(nq <= nq_c), (capacity, Q, K)
        # ... and inside the live plan a queue's last region ends where its path list does: (K - 1) * seg_cap + seg_cap == cap
        assert np.array_equal(K * seg, cap)
        # the last queue's last region, the highest record index a batch forms: below the capacity's allocation
        assert np.all((Q - 1) * K * seg + K * seg <= Q * K * seg_c)
