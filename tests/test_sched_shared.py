"""The shared form of k_primary's schedule in csrc/pt_sched.h — one trace per chunk and run of iterations — without a GPU.

In the shared form a wave keeps ONE residue through its piece (rho = r instead of (r + k) mod wq) and walks chunk outer,
iteration inner, in sub-runs of at most 64 iterations.  k_paths and k_collect read the same buffers as after the per-iteration
form, so the conditions are the same ones: every (queue, iteration, residue) has exactly one owner, and its sub-list receives
the queue's chunks jj = rho, rho + wq, ... in ascending order.  tests/sched_shared_driver.cpp, built with the system compiler,
prints the header's functions over the sweep of tests/test_sched.py plus the run caps; here they are checked by enumeration."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")

QS = (1, 4, 32, 256, 1024)
WQS = (1, 2, 3, 6, 20, 24)
KS = (1, 2, 3, 25, 195, 256)
PRIMARY_PIECES = (0, 1, 2, 3, 4, 7)
SHARES = (1, 2, 8, 64)


def _fields(tokens):
    return {k: int(v) for k, v in (t.split("=") for t in tokens)}


def _ints(line):
    return np.array(line.split(), dtype=np.int64)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [(header fields, [number lines])]} of the driver's output."""
    exe = str(tmp_path_factory.mktemp("sched_shared") / "sched_shared_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_shared_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases = {}
    for line in text.splitlines():
        if line[:1].isalpha() and "=" in line:
            name, *tokens = line.split()
            cases.setdefault(name, []).append((_fields(tokens), []))
            last = cases[name][-1][1]
        else:
            last.append(line)
    return cases


def queue_share(N, Q, q):  # pt_sched.h queue_share, as restated in tests/test_sched.py
    chunks = (N + 63) >> 6
    return (chunks - q + Q - 1) // Q if q < chunks else 0


def test_sub_runs_tile_the_pieces_and_every_sub_list_has_one_owner(out):
    seen = set()
    for f, (strands, runs) in out["shared"]:
        Q, W, K, pp, share, cap = f["Q"], f["W"], f["K"], f["pp"], f["share"], f["cap"]
        wq = W // Q
        seen.add((Q, wq, K, pp, share))
        assert f["max"] == 64 and cap == min(max(share, 1), 64)
        kp = (K + pp - 1) // pp if pp > 1 else K  # strand_plan, with a deal table and not flat: unchanged
        pieces = (K + kp - 1) // kp
        assert (f["kp"], f["pieces"]) == (kp, pieces)
        v = _ints(strands).reshape(W * pieces, 6)
        piece, q, r, k0, k1 = v[:, 0], v[:, 1], v[:, 2], v[:, 4], v[:, 5]
        s = np.arange(W * pieces)
        # piece 0 of strand s < W belongs to wave s = (queue s % Q, rank s // Q); the later pieces follow W at a time
        assert np.all(piece[:W] == 0) and np.array_equal(q[:W], s[:W] % Q) and np.array_equal(r[:W], s[:W] // Q)
        assert np.array_equal(piece, s // W) and np.array_equal(q, s % W % Q) and np.array_equal(r, s % W // Q) and np.all(v[:, 3] == wq)
        assert np.array_equal(k0, piece * kp) and np.array_equal(k1, np.minimum(K, k0 + kp)) and np.all(k0 < k1)
        # sub-runs: consecutive inside their strand from k0 to k1, none empty, none longer than the cap (<= 64), and as few as that allows
        u = _ints(runs).reshape(-1, 3)
        rs, s0, s1 = u[:, 0], u[:, 1], u[:, 2]
        assert np.all(np.diff(rs) >= 0) and np.array_equal(np.unique(rs), s)  # walked strand by strand, every strand has one
        first = np.r_[True, rs[1:] != rs[:-1]]
        last = np.r_[rs[1:] != rs[:-1], True]
        assert np.array_equal(s0[first], k0) and np.array_equal(s1[last], k1)
        assert np.array_equal(s0[~first], s1[:-1][~first[1:]])
        n = s1 - s0
        assert np.all(n >= 1) and np.all(n <= cap) and cap <= 64
        assert np.array_equal(np.bincount(rs), (k1 - k0 + cap - 1) // cap)
        # every (queue, iteration, residue = r) is written by exactly one (strand, sub-run)
        run = np.repeat(np.arange(len(u)), n)
        k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + s0[run]
        visits = np.bincount((q[rs[run]] * K + k) * wq + r[rs[run]], minlength=Q * K * wq)
        assert len(visits) == Q * K * wq and np.all(visits == 1), f
    full = {(Q, wq, K, pp, sh) for Q in QS if Q <= 4 for wq in WQS for K in KS for pp in PRIMARY_PIECES for sh in SHARES}
    assert full <= seen and {c[0] for c in seen} == set(QS)
    for Q in (32, 256, 1024):  # the larger Q: every wq0, K, piece count and cap at least once
        rest = [c for c in seen if c[0] == Q]
        assert {c[1] for c in rest} == set(WQS) and {c[2] for c in rest} == set(KS) and {c[3] for c in rest} == set(PRIMARY_PIECES)
        assert {c[4] for c in rest} == set(SHARES)
    # a piece longer than 64 iterations is cut (K = 195 and 256 in one piece), one of 25 is not
    assert any(f["K"] == 195 and f["pieces"] == 1 and f["share"] == 64 for f, _ in out["shared"])


def test_sub_lists_receive_their_chunks_in_ascending_order(out):
    assert len(out["walk"]) == 6 * 2 * 4 * 3 * 3 * 4
    for f, (line,) in out["walk"]:
        N, Q, wq, K = f["N"], f["Q"], f["wq"], f["K"]
        v = _ints(line).reshape(-1, 4) if line.strip() else np.zeros((0, 4), dtype=np.int64)
        q, k, rho, jj = v.T
        chunks = (N + 63) // 64
        assert len(v) == K * chunks  # every chunk of the tile once per iteration
        # stable sort by sub-list: what each one receives, in the order the owner appends it
        key = (q * K + k) * wq + rho
        order = np.argsort(key, kind="stable")
        key, jj = key[order], jj[order]
        at = 0
        for qq in range(Q):
            my_nq = queue_share(N, Q, qq)
            for kk in range(K):
                for rr in range(wq):
                    want = np.arange(rr, my_nq, wq)  # the residue's chunks, ascending: the per-iteration form's sub-list (q, k, rho)
                    got = jj[at:at + len(want)]
                    assert np.all(key[at:at + len(want)] == (qq * K + kk) * wq + rr) and np.array_equal(got, want), (f, qq, kk, rr)
                    at += len(want)
        assert at == len(v)


def test_form_switch_and_automatic_pieces(out):
    for f, _ in out["form"]:
        assert f["shares"] == int(f["share"] > 1 and not f["aa"] and not f["flat"])  # jitter and the flat lists keep the per-iteration form
        assert f["cap"] == min(max(f["share"], 1), 64)
    assert len(out["auto_shared"]) == len(KS) * 7 * 7
    for f, _ in out["auto_shared"]:
        # pt_api.cpp run_batch: two pieces, more when K needs more than two runs of 64 anyway; never more than iterations
        assert f["pieces"] == max(1, min(max(2, -(-f["K"] // 64)), f["K"]))
