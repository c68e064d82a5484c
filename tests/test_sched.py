"""The work distribution in csrc/pt_sched.h — which wave traces which sample, where a record or a counter lives — without a GPU.

The kernels and the host take these numbers from that header, so what can still go wrong is the header itself.
tests/sched_driver.cpp, built with the system compiler, prints every function for a sweep of (N, Q, wq0, K, pieces); here the
schedule's conditions are checked by enumeration (every pixel, every (queue, iteration, residue), every depth-1 rank has exactly
one owner; every queue keeps a wave; the deal table's regions tile its words), and every quantity must equal the closed form the
kernels and pt_api.cpp spelled out inline before the header existed (restated below from that source), so that the same waves
still trace the same samples."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")

NS = (1, 63, 64, 65, 700, 4097, 259200, 2073600)
QS = (1, 4, 32, 256, 1024)
WQS = (1, 2, 3, 6, 20, 24)
KS = (1, 2, 3, 25, 195, 256)
PRIMARY_PIECES = (0, 1, 2, 3, 4, 7)


def _fields(tokens):
    return {k: int(v) for k, v in (t.split("=") for t in tokens)}


def _ints(line):
    return np.array(line.split(), dtype=np.int64)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [(header fields, [number lines])]} of the driver's output."""
    exe = str(tmp_path_factory.mktemp("sched") / "sched_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases = {}
    for line in text.splitlines():
        if line[0].isalpha() and "=" in line:
            name, *tokens = line.split()
            cases.setdefault(name, []).append((_fields(tokens), []))
            last = cases[name][-1][1]
        else:
            last.append(line)
    return cases


# ── the closed forms of the parent commit, restated ───────────────────────────────────────────────────────────────────────────
def queue_share(N, Q, q):  # pt_kernels.hip queue_share
    chunks = (N + 63) >> 6
    my_nq = (chunks - q + Q - 1) // Q if q < chunks else 0
    last_q = (chunks - 1) % Q
    return my_nq, my_nq * 64 - ((64 - (N & 63)) if (q == last_q and (N & 63)) else 0)


def collect_gap(my_nq, my_pixels, wq0):  # pt_output.inc collect_body
    g0 = g1 = 0
    missing = my_nq * 64 - my_pixels
    if missing > 0:
        quo, rem, rho = my_nq // wq0, my_nq % wq0, (my_nq - 1) % wq0
        g1 = ((rho * quo + min(rho, rem)) + (quo + (1 if rho < rem else 0))) * 64
        g0 = g1 - missing
    return g0, g1


def paths_piece(nextp, total, wq, ps0, pieces_per_wave, ps_min):  # pt_kernels.hip k_paths, "on to the wave's next piece"
    start, sz = total, ps0
    if nextp >= 0:
        start = 0
        level = nextp // wq
        idx = nextp - level * wq
        while level > 0 and start < total:
            start += wq * sz
            sz = max(sz - sz // pieces_per_wave, ps_min)
            level -= 1
        start += idx * sz
    return (start, min(start + sz, total)) if start < total else None


# ── ptd::Queues::deal ─────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_deal_map_regions_tile_the_words(out):
    assert [f["Q"] for f, _ in out["dealmap"]] == list(QS)
    for m, _ in out["dealmap"]:
        Q = m["Q"]
        # (first word, last word) of the five regions, in order: disjoint, consecutive, from 0 to words
        regions = [(m["first0"], m["firstQ"]), (m["time0"], m["timeL"]), (m["strand"], m["strand"]), (m["piece0"], m["pieceL"]), (m["rays0"], m["raysL"])]
        lengths = [Q + 1, Q, 1, Q, Q]
        end = 0
        for (a, b), n in zip(regions, lengths):
            assert a == end and b == a + n - 1, (m, a, b)
            end = b + 1
        assert end == m["words"] and m["made_for"] == m["firstQ"]
        # the parent's offsets: deal[0 .. Q], deal[Q + 1 + q], deal[2 Q + 1], deal[2 Q + 2 + q], deal[3 Q + 2 + q]; 4 Q + 2 words
        assert (m["first0"], m["made_for"], m["time0"], m["strand"], m["piece0"], m["rays0"], m["words"]) == (0, Q, Q + 1, 2 * Q + 1, 2 * Q + 2, 3 * Q + 2, 4 * Q + 2)


def test_deal_keeps_every_queue_a_wave(out):
    seen = set()
    for f, (work, first) in out["deal"]:
        Q, W = f["Q"], f["W"]
        seen.add((Q, W // Q, f["kind"]))
        work, first = [int(x) for x in work.split()], [int(x) for x in first.split()]
        assert len(work) == Q and len(first) == Q + 1 and sum(work) > 0
        assert first[0] == 0 and first[Q] == W
        assert all(a < b for a, b in zip(first, first[1:])), f  # strictly increasing: queue q has first[q + 1] - first[q] >= 1 waves
        total, before = sum(work), 0
        for q in range(Q + 1):  # pt_output.inc deal_waves
            assert first[q] == q + (W - Q) * before // total
            before += work[q] if q < Q else 0
        assert f["close"] == int(max(work) * W * Q <= total * (W + Q))
    assert seen == {(Q, wq, kind) for Q in QS for wq in WQS for kind in range(9)}
    # one queue holds all the work / some hold none; and both answers of the predicate occur
    assert {f["close"] for f, _ in out["deal"]} == {0, 1}


# ── queue geometry ────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_every_pixel_has_one_queue_chunk_and_lane(out):
    assert [(f["N"], f["Q"]) for f, _ in out["geo"]] == [(N, Q) for N in NS for Q in QS]
    for f, lines in out["geo"]:
        N, Q = f["N"], f["Q"]
        chunks = (N + 63) // 64
        assert len(lines) == Q
        owner = np.zeros(chunks, dtype=np.int64)  # (q, jj) pairs per tile chunk
        sum_nq = sum_pixels = 0
        for q, line in enumerate(lines):
            v = _ints(line[2:])
            my_nq, my_pixels, px = int(v[1]), int(v[2]), v[7:]
            assert v[0] == q and len(px) == my_nq
            assert (my_nq, my_pixels) == queue_share(N, Q, q)
            # chunk jj of queue q is tile chunk q + jj * Q: its first pixel, lanes 0 .. 63 behind it
            assert np.array_equal(px, (q + np.arange(my_nq) * Q) * 64)
            assert np.all(px % 64 == 0) and np.all(px < N)
            owner += np.bincount(px // 64, minlength=chunks)
            # pixels a lane exists for: pl = px + lane < N
            assert int(np.minimum(64, N - px).sum()) == my_pixels
            if my_pixels < 64 * my_nq:  # only the queue holding the tile's last chunk, and only its last chunk
                assert N % 64 and px[-1] // 64 == chunks - 1 and my_pixels == 64 * my_nq - (64 - N % 64)
            if my_nq:
                assert list(v[3:7]) == [px[0], px[0] + 63, px[-1], px[-1] + 63]  # slot li = jj * 64 + lane
            else:
                assert list(v[3:7]) == [-1] * 4
            sum_nq += my_nq
            sum_pixels += my_pixels
        assert np.all(owner == 1)  # with the lanes: every tile pixel has exactly one (q, jj, lane)
        assert sum_nq == chunks and sum_pixels == N


def test_sub_regions_and_the_unused_tail(out):
    assert [(f["N"], f["Q"], f["wq0"]) for f, _ in out["sub"]] == [(N, Q, wq0) for N in NS for Q in QS for wq0 in WQS]
    for f, lines in out["sub"]:
        N, Q, wq0 = f["N"], f["Q"], f["wq0"]
        chunks = (N + 63) // 64
        assert len(lines) == min(Q, chunks + 1)  # the queues with chunks and the first without
        gaps = 0
        for q, line in enumerate(lines):
            v = _ints(line[2:])
            my_nq, my_pixels = queue_share(N, Q, q)
            g0, g1, c, off = int(v[1]), int(v[2]), v[3::2], v[4::2]
            assert v[0] == q and len(c) == wq0
            # residue rho owns the chunks jj = rho, rho + wq0, ...; the sub-regions follow each other from 0 to my_nq
            assert np.array_equal(c, [len(range(rho, my_nq, wq0)) for rho in range(wq0)])
            assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(c)[:-1]) and off[-1] + c[-1] == my_nq
            assert (g0, g1) == collect_gap(my_nq, my_pixels, wq0)
            if N % 64 and q == (chunks - 1) % Q:
                rho = (my_nq - 1) % wq0  # the tile's partial last chunk is the queue's last chunk, jj = my_nq - 1
                assert g1 == (off[rho] + c[rho]) * 64 and g1 - g0 == 64 - N % 64
                gaps += 1
            else:
                assert g0 == g1
        assert gaps == (1 if N % 64 else 0)  # [g0, g1) is empty exactly when N % 64 == 0


def test_host_sizes_waves_and_counter_rows(out):
    assert len(out["plan"]) == len(NS) * len(QS) * len(KS)
    for f, _ in out["plan"]:  # pt_api.cpp plan_batches
        nq = ((f["N"] + 63) // 64 + f["Q"] - 1) // f["Q"]
        assert (f["nq"], f["chunks_per_queue"], f["seg_cap"], f["cap"]) == (nq, nq, nq * 64, f["K"] * nq * 64)
        assert f["nq"] == max(queue_share(f["N"], f["Q"], q)[0] for q in range(f["Q"]))
    assert [(f["Q"], f["W"]) for f, _ in out["waves"]] == [(Q, Q * wq) for Q in QS for wq in WQS]
    for f, (line,) in out["waves"]:
        Q, W = f["Q"], f["W"]
        v = _ints(line).reshape(W, 3)
        w = np.arange(W)
        assert np.array_equal(v[:, 0], w % Q) and np.array_equal(v[:, 1], w // Q) and np.all(v[:, 2] == W // Q)
        assert len({(q, r) for q, r in v[:, :2].tolist()}) == W and v[:, 1].max() == W // Q - 1  # every (queue, rank) once
        assert f["sub_stride"] == W // Q  # pt_api.cpp alloc_batch_buffers, wq_max
    for f, _ in out["cnt"]:  # cnt[per_depth * d + q * cnt_stride], per_depth = Q * cnt_stride
        assert f["first"] == f["Q"] * f["stride"] * f["d"] and f["last"] == f["first"] + (f["Q"] - 1) * f["stride"]


# ── k_primary's strands ───────────────────────────────────────────────────────────────────────────────────────────────────────
def test_every_queue_iteration_residue_has_one_strand(out):
    rho, rho_before = {}, {}
    for f, (line,) in out["rho"]:
        wq = f["wq"]
        v = _ints(line).reshape(wq, f["K"], 2)
        r, k = np.meshgrid(np.arange(wq), np.arange(f["K"]), indexing="ij")
        assert np.array_equal(v[:, :, 0], (r + k) % wq) and np.array_equal(v[:, :, 1], (r + k + wq - 1) % wq)
        assert np.array_equal(v[:, 1:, 1], v[:, :-1, 0])  # the residue of the iteration before
        # in one iteration the queue's wq waves have the wq residues, one each
        assert all(sorted(v[:, kk, 0].tolist()) == list(range(wq)) for kk in range(f["K"]))
        rho[wq], rho_before[wq] = v[:, :, 0], v[:, :, 1]
    assert sorted(rho) == list(WQS)
    seen = set()
    for f, (line,) in out["strands"]:
        Q, W, K, pp = f["Q"], f["W"], f["K"], f["pp"]
        wq = W // Q
        seen.add((Q, wq, K, pp))
        # pt_kernels.hip k_primary
        kp = (K + pp - 1) // pp if pp > 1 and f["deal"] and not f["flat"] else K
        pieces = (K + kp - 1) // kp
        assert (f["kp"], f["pieces"]) == (kp, pieces)
        v = _ints(line).reshape(W * pieces, 6)
        piece, q, r, k0, k1 = v[:, 0], v[:, 1], v[:, 2], v[:, 4], v[:, 5]
        s = np.arange(W * pieces)
        sw = s % W
        assert np.array_equal(piece, s // W) and np.array_equal(q, sw % Q) and np.array_equal(r, sw // Q) and np.all(v[:, 3] == wq)
        assert np.array_equal(k0, piece * kp) and np.array_equal(k1, np.minimum(K, k0 + kp))
        assert np.all(piece[:W] == 0) and np.all(k0 < k1)  # the strands < W are piece 0; no strand is empty
        # every (q, k, rho) is visited by exactly one (strand, k)
        n = k1 - k0
        strand = np.repeat(s, n)
        k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + k0[strand]
        visits = np.bincount((q[strand] * K + k) * wq + rho[wq][r[strand], k], minlength=Q * K * wq)
        assert len(visits) == Q * K * wq and np.all(visits == 1), f
    full = {(Q, wq, K, pp) for Q in QS if Q <= 4 for wq in WQS for K in KS for pp in PRIMARY_PIECES}
    assert full <= seen and {Q for Q, *_ in seen} == set(QS)
    for Q in (32, 256, 1024):  # the larger Q: every wq0, K and piece count at least once
        rest = [c for c in seen if c[0] == Q]
        assert {c[1] for c in rest} == set(WQS) and {c[2] for c in rest} == set(KS) and {c[3] for c in rest} == {0, 1, 2, 3, 4, 7}
    for f, _ in out["auto_pieces"]:  # pt_api.cpp run_batch
        groups = f["K"] * f["nq"] // max(1, f["wq0"])
        assert f["pieces"] == min(4, max(1, groups // 48))
    assert len(out["auto_pieces"]) == len(KS) * 7 * 7


# ── k_paths' falling pieces ───────────────────────────────────────────────────────────────────────────────────────────────────
def test_paths_pieces_tile_the_queue(out):
    swept = set()
    for f, (line,) in out["pieces"]:
        total, wq, count, min_piece = f["total"], f["wq"], f["count"], f["min_piece"]
        if f["deal"] and f["sums"]:
            swept.add((total, wq, count, min_piece))
        # one pack / unpack pair; pt_api.cpp take_scene_and_options, pt_kernels.hip k_paths
        assert f["word"] == count | min_piece << 16 and (f["ucount"], f["umin"]) == (count, min_piece)
        ppw = count if f["deal"] and f["sums"] and count > 1 else 1
        ps0 = max((total + wq * ppw - 1) // (wq * ppw), min_piece)
        assert (f["ppw"], f["ps_min"], f["ps0"]) == (ppw, min_piece, ps0)
        v = _ints(line).reshape(-1, 3)
        assert list(v[0]) == [total, total, 0]  # nextp = -1: none
        v = v[1:]
        some = v[:, 2].astype(bool)
        n = int(some.sum())
        assert not some[n:].any() and len(v) - n == 3 * wq + 3  # every nextp after the first empty one is empty
        assert np.all(v[n:, 0] == total) and np.all(v[n:, 1] == total)
        start, end = v[:n, 0], v[:n, 1]
        for nextp in range(len(v)):  # the loop k_paths had inline
            want = paths_piece(nextp, total, wq, ps0, ppw, min_piece)
            assert (want is None and not some[nextp]) or want == (start[nextp], end[nextp]), (f, nextp)
        if total == 0:
            assert n == 0
        else:  # non-empty, consecutive, disjoint, ending exactly at total
            assert start[0] == 0 and end[-1] == total and np.all(start < end) and np.array_equal(start[1:], end[:-1])
            size = end - start
            level = np.arange(n) // wq
            # one size per level (but for the last piece), not growing from level to level, >= min_piece
            assert all(len(set(size[:-1][level[:-1] == l].tolist())) <= 1 for l in range(level[-1] + 1))
            assert np.all(size[1:-1] <= size[:-2]) and np.all(size[:-1] >= min_piece) and size[-1] <= (size[-2] if n > 1 else ps0)
        assert f["needs_counter"] == int(n > wq)  # a counter exactly when more than the waves' own pieces exist
    assert swept == {(t, wq, c, m) for t in (0, 1, 2, 63, 64, 65, 127, 1000, 4097, 50000) for wq in (1, 2, 3, 6, 24) for c in (1, 2, 3, 4, 8) for m in (1, 3, 64)}
    assert len(swept) == 750 and len(out["pieces"]) > 750  # (+ the forms without a deal table / without chunk sums)
