"""align: the whole path of each read's sDTW alignment, event to reference, on the device (docs/codecs.md §4.17;
slow5tools_amd/csrc/dtw_path_kernels.hip).

The oracle is path_ref of dtw_ref.py: the FULL matrix D of §4.16 in int64 numpy, walked back from (Q - 1, end) with the tie rule.  The device
runs the recurrence over the columns [start, end] only, so every comparison here also checks §4.17's argument that the window is enough.
Everything is integer: lo, hi and status are held to the restatement exactly.  The header's lane step, packing and walk (dtw_dev.h) are
plain C++: they are also compiled for the CPU, 64 lanes in lockstep writing the words the way the kernel lays them out, and held to the
same oracle.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from chain_common import DNA, EMPTY, EVENT, GUARD, MAP_ROW, PATH_ROW, PATH_WIDE, QUERY_SHORT, ROOT, host_build, levels_signal, record, synth_file
from chain_common import gpu  # noqa: F401
from dtw_ref import QLENS, _g_of, _mixed, known_answer_cases, last_lane_batch, path_ref, quant_ref

# ---------------------------------------------------------------------------------------------------------------- not gpu

CALLS = ["s5gpu_sdtw_path_slot_bytes", "s5gpu_sdtw_path_dev", "s5gpu_align_batch"]
STATUSES = ["S5GPU_STATUS_PATH_WIDE", "S5GPU_STATUS_PATH_ROW"]


def test_library_exports_the_align_calls_and_the_tool_is_built(tmp_path):
    from slow5tools_amd import _lib, align, build

    build.build()
    assert os.access(align.S5ALIGN, os.X_OK)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [2, 14, 15]
    # the header declares the calls and the two statuses (a C program that uses them compiles against it alone)
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "slow5gpu.h"\nint main(void){\n'
                   'size_t (*a)(uint32_t, uint32_t) = s5gpu_sdtw_path_slot_bytes;\n'
                   'int (*b)(uint32_t, const int16_t *, uint32_t, const uint32_t *, const int16_t *, uint32_t, const s5gpu_map_row_t *, uint32_t, void *, size_t,'
                   ' int32_t *, int32_t *, int32_t *, void *) = s5gpu_sdtw_path_dev;\n'
                   'int (*c)(uint32_t, const void *const *, const size_t *, int, int, const s5gpu_event_params_t *, const s5gpu_map_params_t *, uint32_t,'
                   ' const int16_t *, uint32_t, s5gpu_map_row_t *, int32_t *, int32_t *, s5gpu_event_t *, int32_t *) = s5gpu_align_batch;\n'
                   'printf("%d %d %d\\n", S5GPU_STATUS_PATH_WIDE, S5GPU_STATUS_PATH_ROW, a && b && c);return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == [str(PATH_WIDE), str(PATH_ROW), "1"]
    assert (_lib.STATUS_PATH_WIDE, _lib.STATUS_PATH_ROW) == (PATH_WIDE, PATH_ROW)


def test_slot_bytes_is_monotone_and_zero_for_refused_arguments():
    from slow5tools_amd import _lib

    f = _lib.lib().s5gpu_sdtw_path_slot_bytes
    for qpitch, wmax in ((0, 100), (1025, 100), (64, 0), (64, (1 << 20) + 1), (0, 0), (1 << 31, 1 << 31)):
        assert f(qpitch, wmax) == 0, (qpitch, wmax)
    pitches, widths = [1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024], [1, 2, 15, 16, 17, 64, 250, 1000, 4096, 1 << 20]
    t = np.array([[f(p, w) for w in widths] for p in pitches], dtype=np.int64)
    assert (t > 0).all() and (t % 256 == 0).all()
    assert (np.diff(t, axis=0) >= 0).all() and (np.diff(t, axis=1) >= 0).all()
    assert t[0, 0] < t[-1, 0] and t[0, 0] < t[0, -1]
    # 2 bits per cell of 64 lanes over wmax + 63 steps, in whole words of 16 / G steps
    assert f(64, 1) == 256 * 4 and f(1024, 1) == 256 * 64 and f(256, 1000) == 256 * ((1063 + 3) // 4)


def test_the_passes_option_takes_1_to_3():
    from slow5tools_amd import _lib

    L = _lib.lib()
    for bad in (0, 4, -1):
        assert L.s5gpu_set_option(b"sdtw_path_passes", bad) == -1
    for good in (1, 2, 3):                                                 # (3 last: the default)
        assert L.s5gpu_set_option(b"sdtw_path_passes", good) == 0


PATH_HOST = r'''
// The code of k_sdtw_dirs and k_sdtw_trace that lives in dtw_dev.h, on the CPU: 64 lanes in lockstep over the window, the words written the
// way the kernel lays them out ([word][lane]), then the header's walk over them.  The row comes from the lane code of k_sdtw (as in
// tests/test_map.py).  in.bin holds cases (Q, R, G, q, r); out.bin gets cost, start, end, status, lo[Q], hi[Q] of each.
#define S5_DTW_HOST
#include "dtw_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace dtwk;
static void shift_up1(const uint32_t *v, uint32_t fill, uint32_t *out) { for (int l = 63; l >= 1; l--) out[l] = v[l - 1]; out[0] = fill; }

template <int G, int KB>
static U4 row_of(const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R) {
    std::vector<Lane<G, true> > L(64);
    uint32_t rcur[64], v[64], r[64], up[64], sup[64];
    for (uint32_t l = 0; l < 64; l++) {
        lane_init(L[l], l == 0);
        rcur[l] = 0;
        for (int k = 0; k < G; k++) { const uint32_t row = l * G + k; L[l].q[k] = biased(row < Q ? q[row] : (int16_t)0); }
    }
    const uint32_t last = (Q - 1) / G, steps = R + last;
    for (uint32_t t = 0; t < steps; t++) {
        shift_up1(rcur, biased(t < R ? ref[t] : (int16_t)0), r);
        for (int l = 0; l < 64; l++) { rcur[l] = r[l]; v[l] = L[l].d[G - 1]; }
        shift_up1(v, 0u, up);
        for (int l = 0; l < 64; l++) v[l] = (uint32_t)L[l].s[G - 1];
        shift_up1(v, t + 1, sup);
        for (uint32_t l = 0; l < 64; l++) { lane_step(L[l], r[l], up[l], (int32_t)sup[l]); lane_best<G, true, KB>(L[l], t - l, R); }
    }
    return result_row(L[last].best, Q, L[last].best_start, L[last].best_end);
}
template <int G, int KB = 0>
struct Pick {
    static U4 go(int kb, const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R) {
        if (kb == KB) return row_of<G, KB>(q, Q, ref, R);
        if constexpr (KB + 1 < G) return Pick<G, KB + 1>::go(kb, q, Q, ref, R);
        abort();
    }
};

// k_sdtw_dirs over the window [start, start + W): whole words, every lane at every step
template <int G>
static void dirs(const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t W, uint32_t *slot, uint32_t slot_words) {
    const uint32_t SPW = 16 / G;
    std::vector<Lane<G, false> > L(64);
    uint32_t rcur[64], v[64], r[64], up[64], word[64];
    for (uint32_t l = 0; l < 64; l++) {
        lane_init(L[l], l == 0);
        rcur[l] = 0;
        for (int k = 0; k < G; k++) { const uint32_t row = l * G + k; L[l].q[k] = biased(row < Q ? q[row] : (int16_t)0); }
    }
    const uint32_t last = (Q - 1) / G;
    uint32_t nw = path_words(G, W + last);
    if (nw > slot_words) abort();
    for (uint32_t w = 0; w < nw; w++) {
        for (int l = 0; l < 64; l++) word[l] = 0;
        for (uint32_t s = 0; s < SPW; s++) {
            const uint32_t t = w * SPW + s;
            shift_up1(rcur, biased(t < W ? ref[t] : (int16_t)0), r);
            for (int l = 0; l < 64; l++) { rcur[l] = r[l]; v[l] = L[l].d[G - 1]; }
            shift_up1(v, 0u, up);
            for (int l = 0; l < 64; l++) word[l] = path_pack(word[l], lane_step_dirs(L[l], r[l], up[l]), s, G);
        }
        for (int l = 0; l < 64; l++) slot[(size_t)w * 64 + l] = word[l];
    }
}

static int one_case(FILE *f, FILE *o) {
    uint32_t Q, R, G;
    if (fread(&Q, 4, 1, f) != 1) return 1;
    if (fread(&R, 4, 1, f) != 1 || fread(&G, 4, 1, f) != 1 || Q < 1 || Q > 64 * G || R < 1) return -1;
    std::vector<int16_t> q(Q), r(R);
    if (fread(q.data(), 2, Q, f) != Q || fread(r.data(), 2, R, f) != R) return -1;
    const int kb = (int)((Q - 1) % G);
    U4 row;
    if (G == 1) row = Pick<1>::go(kb, q.data(), Q, r.data(), R);
    else if (G == 2) row = Pick<2>::go(kb, q.data(), Q, r.data(), R);
    else if (G == 4) row = Pick<4>::go(kb, q.data(), Q, r.data(), R);
    else if (G == 8) row = Pick<8>::go(kb, q.data(), Q, r.data(), R);
    else if (G == 16) row = Pick<16>::go(kb, q.data(), Q, r.data(), R);
    else return -1;
    uint32_t W = 0;
    int32_t st = path_row_check(row, Q, R, WMAX, &W);
    std::vector<int32_t> lo(Q, -1), hi(Q, -1);
    if (st == 0) {
        const uint32_t slot_words = path_words(G, W + 63);
        // exactly the slot, filled with ones: a word the walk must not read would give a code of 3
        uint32_t *slot = (uint32_t *)malloc((size_t)slot_words * 256);
        if (!slot) return -1;
        memset(slot, 0xFF, (size_t)slot_words * 256);
        const int16_t *wref = r.data() + (int32_t)row.z;
        if (G == 1) dirs<1>(q.data(), Q, wref, W, slot, slot_words);
        else if (G == 2) dirs<2>(q.data(), Q, wref, W, slot, slot_words);
        else if (G == 4) dirs<4>(q.data(), Q, wref, W, slot, slot_words);
        else if (G == 8) dirs<8>(q.data(), Q, wref, W, slot, slot_words);
        else dirs<16>(q.data(), Q, wref, W, slot, slot_words);
        st = path_walk(slot, slot_words, G, Q, W, (int32_t)row.z, lo.data(), hi.data());
        free(slot);
    }
    const int32_t head[4] = {(int32_t)row.x, (int32_t)row.z, (int32_t)row.w, st};
    fwrite(head, 4, 4, o);
    fwrite(lo.data(), 4, Q, o);
    fwrite(hi.data(), 4, Q, o);
    return 0;
}

// A decision buffer whose walk reaches row 0 right of window column 0: Q = 3 rows in a window of W = 2 columns, every code 1 ((i - 1, j)),
// so from (2, 1) it goes straight up to (0, 1).  Prints path_walk's status, and what path_walk_from says of the same buffer.
static int row0_case(void) {
    const uint32_t G = 1, Q = 3, W = 2, slot_words = path_words(G, W + 63);
    std::vector<uint32_t> slot((size_t)slot_words * 64, 0x55555555u);
    int32_t lo[3] = {-7, -7, -7}, hi[3] = {-7, -7, -7}, lo2[3], hi2[3], start = -7;
    const int32_t st = path_walk(slot.data(), slot_words, G, Q, W, 10, lo, hi);
    const int32_t st2 = path_walk_from(slot.data(), slot_words, G, Q, W, 10, W - 1, lo2, hi2, &start);
    printf("%d %d %d\n", st, st2, start);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "row0") == 0) return row0_case();
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    for (;;) {
        const int rc = one_case(f, o);
        if (rc < 0) return 1;
        if (rc > 0) break;
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def _window_case(rng, Q, W, lo, hi):
    """a query and a reference whose window is W wide by construction: W distinct levels far from everything else in the reference, the query
    their sequence with the rows shared out among them (Q >= W), or a query of one level on a flat reference (W = 1)"""
    assert Q >= W
    piece = (np.arange(W) * 40 - 20 * W).astype(np.int64)
    counts = np.full(W, Q // W)
    counts[:Q % W] += 1
    q = np.repeat(piece, counts)
    r = np.concatenate([np.full(7, 30000), piece, np.full(5, -30000)])
    return q.astype(np.int16), r.astype(np.int16)


def host_cases():
    rng = np.random.default_rng(17)
    cases = []
    for Q in QLENS[1:]:                                                    # every G, Q on both sides of every lane boundary
        R = int(rng.integers(60, 140))
        cases.append((rng.integers(-127, 128, Q), rng.integers(-127, 128, R), _g_of(Q)))
        cases.append((rng.integers(-1, 2, Q), rng.integers(-1, 2, R), _g_of(Q)))
    for W in (1, 2, 63, 64, 65, 129):                                      # windows of a known width
        q, r = _window_case(rng, max(W, 3) + 4, W, -127, 127)
        cases.append((q, r, _g_of(len(q))))
        q, r = _window_case(rng, 300, W, -127, 127)
        cases.append((q, r, 8))
    cases.append((rng.integers(-32768, 32768, 1024), rng.integers(-32768, 32768, 90), 16))     # full range
    cases.append((rng.integers(-127, 128, 5), rng.integers(-127, 128, 70), 4))                  # a G above the smallest: most lanes idle
    cases.append((rng.integers(-1, 2, 130), rng.integers(-1, 2, 64), 16))
    return [(np.asarray(q, dtype=np.int16), np.asarray(r, dtype=np.int16), g) for q, r, g in cases]


HAND_MADE = [([1, 2, 3], [7, 7, 1, 2, 3, 7], [2, 3, 4], [2, 3, 4]),
             ([1, 1, 1, 2, 2], [1, 2], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1]),
             ([3, 3], [0], [0, 0], [0, 0]),
             ([5], [4, 4, 4, 4], [0], [0]),                                # one value on a flat reference: W = 1
             ([1, 5, 9], [1, 5, 5, 5, 9], [0, 1, 4], [0, 3, 4])]           # the event of 5 spans the columns 1 .. 3: lo < hi


def _build_path_host(tmp_path, extra=()):
    return host_build(tmp_path, "path_host", PATH_HOST, ["-O1", "-std=c++17", "-ffp-contract=off"], extra)


def test_restatement_on_hand_made_paths():
    for q, r, lo, hi in HAND_MADE:
        c, l, h = path_ref(q, r)
        assert l.tolist() == lo and h.tolist() == hi, (q, r)
    assert path_ref([5], [4, 4, 4, 4])[0] == 1 and path_ref([1, 5, 9], [1, 5, 5, 5, 9])[0] == 0 and path_ref([3, 3], [0])[0] == 6
    # ties: all zeros; the smallest end, and from there the diagonal while it can
    c, l, h = path_ref([0, 0, 0], [0, 0, 0, 0, 0])
    assert (c, l.tolist(), h.tolist()) == (0, [0, 0, 0], [0, 0, 0])
    c, l, h = path_ref([0, 0, 0], [5, 0, 0, 0])
    assert (c, l.tolist(), h.tolist()) == (0, [1, 1, 1], [1, 1, 1])
    # the window cases have the width they were built for
    for W in (1, 2, 63, 64, 65, 129):
        q, r = _window_case(None, 300, W, -127, 127)
        c, l, h = path_ref(q, r)
        assert c == 0 and l[0] == 7 and h[-1] == 7 + W - 1


def test_the_path_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """lane_step_dirs, path_pack, path_cell and path_walk of dtw_dev.h as g++ compiles them: every G with Q on both sides of every lane
    boundary, windows of 1, 2, 63, 64, 65 and 129 columns, values of +-127 and of {-1, 0, 1} (ties), the full int16 range at Q = 1024, a G
    above the smallest, and the hand-made paths"""
    cases = host_cases() + [(np.array(q, dtype=np.int16), np.array(r, dtype=np.int16), 1) for q, r, lo, hi in HAND_MADE]
    exe = _build_path_host(tmp_path)
    with open(tmp_path / "in.bin", "wb") as fh:
        for q, r, g in cases:
            fh.write(struct.pack("<III", len(q), len(r), g) + q.tobytes() + r.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw, at = (tmp_path / "out.bin").read_bytes(), 0
    widths = set()
    for q, r, g in cases:
        Q = len(q)
        cost, start, end, st = np.frombuffer(raw, np.int32, 4, at).tolist()
        lo, hi = np.frombuffer(raw, np.int32, Q, at + 16), np.frombuffer(raw, np.int32, Q, at + 16 + 4 * Q)
        at += 16 + 8 * Q
        c, wl, wh = path_ref(q, r)
        assert (cost, start, end, st) == (c, int(wl[0]), int(wh[-1]), 0), (Q, len(r), g)
        assert np.array_equal(lo, wl) and np.array_equal(hi, wh), (Q, len(r), g)
        widths.add(end - start + 1)
    assert at == len(raw) and {1, 2, 63, 64, 65, 129} <= widths
    for (q, r, lo, hi), case in zip(HAND_MADE, cases[-len(HAND_MADE):]):
        assert path_ref(case[0], case[1])[1].tolist() == lo
    # a walk that arrives in row 0 right of window column 0 is refused by path_walk; path_walk_from takes it, and names the column (10 + 1)
    assert subprocess.check_output([exe, "row0"], text=True).split() == [str(PATH_ROW), "0", "11"]


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3) of the two device-pointer calls: the pointers are never dereferenced on the host, so
    made-up aligned addresses serve"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    P = 1 << 20                                                            # an aligned address

    def path(n=4, q=P, pitch=64, ql=P, ref=P, R=100, rows=P, wmax=256, scratch=P, sb=1 << 30, lo=P, hi=P, st=P):
        return L.s5gpu_sdtw_path_dev(n, q, pitch, ql, ref, R, rows, wmax, scratch, sb, lo, hi, st, None)
    assert path(pitch=0) == -1 and path(pitch=1025) == -1 and path(R=0) == -1 and path(R=1 << 31) == -1 and path(ref=None) == -1
    assert path(wmax=0) == -1 and path(wmax=(1 << 20) + 1) == -1
    for name in ("q", "ql", "rows", "scratch", "lo", "hi", "st"):
        assert path(**{name: None}) == -1, name
    assert path(q=P + 1) == -1 and path(ql=P + 2) == -1 and path(ref=P + 1) == -1 and path(rows=P + 8) == -1 and path(scratch=P + 8) == -1
    assert path(lo=P + 2) == -1 and path(hi=P + 1) == -1 and path(st=P + 2) == -1
    slot = L.s5gpu_sdtw_path_slot_bytes(64, 256)
    assert slot > 0 and path(sb=slot - 1) == -3 and path(sb=0) == -3
    assert path(n=0) == 0 and path(n=0, sb=0) == 0                        # nothing to do: nothing is launched
    # the batch call: the cases of s5gpu_map_batch, and wmax
    vp = C.c_void_p
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (vp * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    h_ref = np.zeros(100, dtype=np.int16)
    h_rows, h_lo, h_hi = np.full(16, 0xA5, dtype=np.uint8), np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32)
    h_st = np.full(1, -7, dtype=np.int32)

    def batch(pr=(0, 64, 10, 32.0, 127, 1), ev=DNA, wmax=256, R=100, ref=True, ev_null=False, mp_null=False, rows=True, lo=True, methods=(1, 1)):
        e, p = _lib.EventParams(*ev), _lib.MapParams(*pr)
        return L.s5gpu_align_batch(1, rec_p, rl, methods[0], methods[1], None if ev_null else C.byref(e), None if mp_null else C.byref(p), wmax,
                                   h_ref.ctypes.data_as(vp) if ref else None, R, h_rows.ctypes.data_as(vp) if rows else None,
                                   h_lo.ctypes.data_as(vp) if lo else None, h_hi.ctypes.data_as(vp), None, h_st.ctypes.data_as(vp))
    nan = float("nan")
    for pr in ((0, 0, 1, 32.0, 127, 1), (0, 1025, 1, 32.0, 127, 1), (0, 64, 0, 32.0, 127, 1), (0, 64, 65, 32.0, 127, 1), (0, 64, 10, nan, 127, 1),
               (0, 64, 10, 0.0, 127, 1), (0, 64, 10, 32.0, 0, 1), (0, 64, 10, 32.0, 32768, 1)):
        assert batch(pr=pr) == -1, pr
    assert batch(wmax=0) == -1 and batch(wmax=(1 << 20) + 1) == -1 and batch(R=0) == -1 and batch(ref=False) == -1
    assert batch(ev_null=True) == -1 and batch(mp_null=True) == -1 and batch(rows=False) == -1 and batch(lo=False) == -1
    assert batch(ev=(3, 3, 1.4, 9.0, 0.2)) == -1 and batch(methods=(9, 1)) == -1 and batch(methods=(1, 9)) == -1
    assert (h_rows == 0xA5).all() and (h_lo == -7).all() and (h_hi == -7).all() and (h_st == -7).all()


# ---------------------------------------------------------------------------------------------------------------- gpu

def _rows_dev(env, qm, qlens, ref, pitch, want_start=True):
    torch = env.torch
    d_q = torch.from_numpy(np.ascontiguousarray(qm)).to("cuda")
    d_ql = torch.from_numpy(np.asarray(qlens, dtype=np.int32)).to("cuda")
    d_r = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16)).to("cuda")
    d_rows = torch.zeros((len(qlens), 4), dtype=torch.int32, device="cuda")
    env.lib.check(env.L.s5gpu_sdtw_dev(len(qlens), d_q.data_ptr(), pitch, d_ql.data_ptr(), d_r.data_ptr(), len(ref), int(want_start), d_rows.data_ptr(), None),
                  "s5gpu_sdtw_dev")
    return d_q, d_ql, d_r, d_rows


def _run_path(env, qm, qlens, ref, wmax, pitch=None, scratch_bytes=None, rows=None, expect=0):
    """s5gpu_sdtw_dev with want_start, then s5gpu_sdtw_path_dev with 0x5A guard rows around lo, hi and status and a guard behind the scratch
    -> (lo [n, pitch], hi, status, rows).  rows: a MAP_ROW array to use in place of what s5gpu_sdtw_dev wrote.  Guards and inputs are checked
    here."""
    torch, L = env.torch, env.L
    n = len(qlens)
    pitch = qm.shape[1] if pitch is None else pitch
    d_q, d_ql, d_r, d_rows = _rows_dev(env, qm, qlens, ref, pitch)
    if rows is not None:
        d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32).reshape(n, 4)).to("cuda")
    torch.cuda.synchronize()
    h_rows = d_rows.cpu().numpy().copy()
    slot = L.s5gpu_sdtw_path_slot_bytes(pitch, wmax)
    sb = slot * n if scratch_bytes is None else scratch_bytes
    d_scr = torch.full((sb // 4 + 64,), GUARD, dtype=torch.int32, device="cuda")
    d_lo = torch.full(((n + 2) * pitch,), GUARD, dtype=torch.int32, device="cuda")
    d_hi = torch.full(((n + 2) * pitch,), GUARD, dtype=torch.int32, device="cuda")
    d_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda")
    assert d_scr.data_ptr() % 16 == 0
    rc = L.s5gpu_sdtw_path_dev(n, d_q.data_ptr(), pitch, d_ql.data_ptr(), d_r.data_ptr(), len(ref), d_rows.data_ptr(), wmax, d_scr.data_ptr(), sb,
                               d_lo.data_ptr() + 4 * pitch, d_hi.data_ptr() + 4 * pitch, d_st.data_ptr() + 4, None)
    torch.cuda.synchronize()
    lo, hi, st, scr = d_lo.cpu().numpy(), d_hi.cpu().numpy(), d_st.cpu().numpy(), d_scr.cpu().numpy()
    assert rc == expect
    if rc != 0:
        assert (lo == GUARD).all() and (hi == GUARD).all() and (st == GUARD).all() and (scr == GUARD).all()      # nothing was launched
        return None
    for a, w in ((lo, pitch), (hi, pitch), (st, 1)):
        assert (a[:w] == GUARD).all() and (a[-w:] == GUARD).all(), "a guard row was written"
    assert (scr[sb // 4:] == GUARD).all(), "the guard behind the scratch was written"
    assert np.array_equal(d_q.cpu().numpy(), qm) and np.array_equal(d_r.cpu().numpy(), np.asarray(ref, dtype=np.int16))
    assert np.array_equal(d_ql.cpu().numpy(), np.asarray(qlens, dtype=np.int32)) and np.array_equal(d_rows.cpu().numpy(), h_rows)
    return lo[pitch:-pitch].reshape(n, pitch).copy(), hi[pitch:-pitch].reshape(n, pitch).copy(), st[1:-1].copy(), h_rows.view(MAP_ROW).reshape(-1)


def _want(qm, qlens, ref, pitch):
    """lo, hi [n, pitch] and the rows of path_ref, -1 behind qlen"""
    n = len(qlens)
    lo, hi, rows = np.full((n, pitch), -1, dtype=np.int32), np.full((n, pitch), -1, dtype=np.int32), np.zeros(n, dtype=MAP_ROW)
    for i, Q in enumerate(qlens):
        Q = min(Q, pitch)
        if Q == 0:
            rows[i] = EMPTY
            continue
        c, l, h = path_ref(np.asarray(qm[i])[:Q], ref)
        lo[i, :Q], hi[i, :Q], rows[i] = l, h, (c, Q, l[0], h[-1])
    return lo, hi, rows


def _check(got, want, what, status=None):
    lo, hi, st, rows = got
    wl, wh, wr = want
    assert rows.tolist() == wr.tolist(), what
    assert st.tolist() == ([0] * len(st) if status is None else status), what
    for name, g, w in (("lo", lo, wl), ("hi", hi, wh)):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


@pytest.fixture(scope="module")
def mixed():
    """the mixed batches and their restatements, computed once: {(alphabet, R): (qm, ref, want)}"""
    rng = np.random.default_rng(4)
    out = {}
    for name, a, b in (("pm127", -127, 127), ("ties", -1, 1)):
        qm = _mixed(rng, a, b)
        for R in (65, 129, 500):
            ref = np.random.default_rng(100 + R).integers(a, b + 1, R).astype(np.int16)
            out[name, R] = (qm, ref, _want(qm, QLENS, ref, 1024))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("R", [65, 129, 500])
@pytest.mark.parametrize("name", ["pm127", "ties"])
def test_path_is_exact_on_a_mixed_batch(gpu, mixed, name, R):
    qm, ref, want = mixed[name, R]
    got = _run_path(gpu, qm, QLENS, ref, wmax=R)
    _check(got, want, (name, R))
    lo, hi, st, rows = got
    assert st[0] == 0 and (lo[0] == -1).all() and (hi[0] == -1).all()      # qlen = 0: status 0 and no path
    for i, Q in enumerate(QLENS):
        assert (lo[i, Q:] == -1).all() and (hi[i, Q:] == -1).all() and (lo[i, :Q] >= 0).all()


@pytest.mark.gpu
def test_path_every_row_of_the_last_lane(gpu):
    qm, ql = last_lane_batch()
    ref = np.random.default_rng(42).integers(-127, 128, 129).astype(np.int16)
    want = _want(qm, ql, ref, 1024)
    assert want[2]["qlen"].tolist() == ql and (want[2]["cost"] < 2 ** 26).all() and (want[0][:, 0] >= 0).all()      # every read has a path
    _check(_run_path(gpu, qm, ql, ref, wmax=129), want, "every row of the last lane")


@pytest.mark.gpu
def test_path_in_groups_equals_the_ungrouped_run(gpu, mixed):
    qm, ref, want = mixed["pm127", 129]
    slot = gpu.L.s5gpu_sdtw_path_slot_bytes(1024, 129)
    whole = _run_path(gpu, qm, QLENS, ref, wmax=129)
    _check(whole, want, "ungrouped")
    for sb in (3 * slot, 3 * slot + 100, slot, 2 * slot - 1):              # 6 groups the last of one read; 16 groups of one
        got = _run_path(gpu, qm, QLENS, ref, wmax=129, scratch_bytes=sb)
        _check(got, want, sb)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], whole[:3]))
    assert _run_path(gpu, qm, QLENS, ref, wmax=129, scratch_bytes=slot - 1, expect=-3) is None


@pytest.mark.gpu
def test_path_status_wide_and_unusable_rows(gpu):
    rng = np.random.default_rng(23)
    ref_k, cases = known_answer_cases()
    # the span is known by construction: every level of a slice held 3 times, W = the slice's length
    a, W = 300, 70
    ref = ref_k[200:500].copy()
    wide = np.repeat(ref[a - 200:a - 200 + W], 3).astype(np.int16)
    Q = len(wide)
    qm = rng.integers(-100, 101, (5, Q)).astype(np.int16)
    qm[2] = wide
    ql = [30, 40, Q, 25, 3]                                                # (the neighbours are short: a random query's span is about its length)
    want = _want(qm, ql, ref, Q)
    spans = want[2]["end"] - want[2]["start"] + 1
    assert spans[2] == W and want[2]["cost"][2] == 0 and (spans[[0, 1, 3, 4]] < W - 1).all()
    _check(_run_path(gpu, qm, ql, ref, wmax=W), want, "wmax = W")
    lo, hi, st, rows = _run_path(gpu, qm, ql, ref, wmax=W - 1)
    assert st.tolist() == [0, 0, PATH_WIDE, 0, 0] and (lo[2] == -1).all() and (hi[2] == -1).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(lo[keep], want[0][keep]) and np.array_equal(hi[keep], want[1][keep]) and rows.tolist() == want[2].tolist()
    # unusable rows among valid reads: made without want_start, end >= R, start > end, a wrong qlen
    d_q, d_ql, d_r, d_rows = _rows_dev(gpu, qm, ql, ref, Q, want_start=False)
    gpu.torch.cuda.synchronize()
    no_start = d_rows.cpu().numpy().view(MAP_ROW).reshape(-1)
    assert (no_start["start"] == -1).all() and np.array_equal(no_start["end"], want[2]["end"])
    good = want[2]
    for what, at, row in (("no want_start", 1, tuple(no_start[1])), ("end >= R", 0, (good[0]["cost"], ql[0], good[0]["start"], len(ref))),
                          ("end far", 3, (good[3]["cost"], ql[3], good[3]["start"], 0x7FFFFFFF)),
                          ("start > end", 2, (0, Q, good[2]["end"] + 1, good[2]["end"])), ("wrong qlen", 4, (good[4]["cost"], 4, good[4]["start"], good[4]["end"])),
                          ("qlen 0", 0, EMPTY)):
        rows_in = good.copy()
        rows_in[at] = row
        lo, hi, st, rows = _run_path(gpu, qm, ql, ref, wmax=W, rows=rows_in)
        keep = [i for i in range(5) if i != at]
        assert st.tolist() == [PATH_ROW if i == at else 0 for i in range(5)], what
        assert (lo[at] == -1).all() and (hi[at] == -1).all(), what
        assert np.array_equal(lo[keep], want[0][keep]) and np.array_equal(hi[keep], want[1][keep]), what


@pytest.mark.gpu
def test_path_many_waves_and_workgroups(gpu):
    rng = np.random.default_rng(8)
    qm, ref = rng.integers(-127, 128, (200, 64)).astype(np.int16), rng.integers(-127, 128, 129).astype(np.int16)
    want = _want(qm, [64] * 200, ref, 64)
    _check(_run_path(gpu, qm, [64] * 200, ref, wmax=129), want, "n = 200")
    assert len(set(want[2]["end"].tolist())) > 20
    # a pitch below the matrix's own: the queries are the first 40 values of every 64, qlen beyond the pitch is the pitch
    q40 = qm.reshape(320, 40)
    want = _want(q40, [40] * 320, ref, 40)
    _check(_run_path(gpu, q40, [40] * 319 + [64], ref, wmax=129, pitch=40), want, "pitch 40")


@pytest.mark.gpu
def test_path_dev_finds_the_known_paths(gpu):
    """the warped slices of dtw_ref.py: cost 0, and event rows lo = hi = the column of their level, each held `rep` times"""
    torch = gpu.torch
    ref, cases = known_answer_cases()
    assert len(cases) >= 20
    pitch = max(len(q) for q, a, Q, rep in cases)
    qm = np.zeros((len(cases), pitch), dtype=np.int16)
    for i, (q, a, Q, rep) in enumerate(cases):
        qm[i, :len(q)] = q
    ql = np.array([len(q) for q, a, Q, rep in cases], dtype=np.int32)
    d_q, d_ql, d_r = torch.from_numpy(qm).to("cuda"), torch.from_numpy(ql).to("cuda"), torch.from_numpy(ref).to("cuda")
    rows = gpu.map.sdtw_dev(d_q, d_ql, d_r, want_start=True)
    lo, hi, st = gpu.align.path_dev(d_q, d_ql, d_r, rows)
    assert lo.is_cuda and lo.dtype == torch.int32 and tuple(lo.shape) == (len(cases), pitch) and tuple(st.shape) == (len(cases),)
    lo, hi, st = lo.cpu().numpy(), hi.cpu().numpy(), st.cpu().numpy()
    assert rows.cpu().numpy().view(MAP_ROW).reshape(-1).tolist() == [(0, len(q), a, a + Q - 1) for q, a, Q, rep in cases]
    assert not st.any()
    for i, (q, a, Q, rep) in enumerate(cases):
        col = np.repeat(np.arange(a, a + Q), rep)
        assert np.array_equal(lo[i, :len(q)], col) and np.array_equal(hi[i, :len(q)], col), i
        assert (lo[i, len(q):] == -1).all() and (hi[i, len(q):] == -1).all()
    # wmax below the widest span: those reads have no path, the others keep theirs
    w = sorted(Q for q, a, Q, rep in cases)[len(cases) // 2]
    lo2, hi2, st2 = (t.cpu().numpy() for t in gpu.align.path_dev(d_q, d_ql, d_r, rows, wmax=w))
    assert st2.tolist() == [PATH_WIDE if Q > w else 0 for q, a, Q, rep in cases] and 0 < (st2 != 0).sum() < len(cases)
    for i in range(len(cases)):
        assert np.array_equal(lo2[i], lo[i] if st2[i] == 0 else np.full(pitch, -1)) and np.array_equal(hi2[i], hi[i] if st2[i] == 0 else np.full(pitch, -1))


@pytest.mark.gpu
def test_align_end_to_end_on_a_synthetic_file(gpu, tmp_path):
    """read_align, align_dev and file_align (s5align) on level signals, one record corrupt and one read too short: the same rows, lo, hi and
    statuses, equal to path_ref on the queries that queries_dev makes, the events the rows [skip, skip + qlen) of events_dev"""
    torch, al = gpu.torch, gpu.align
    rng = np.random.default_rng(41)
    lengths = [3000, 500, 40, 5000, 1500, 2500]
    recs = [record(i, levels_signal(n, rng)) for i, n in enumerate(lengths)]
    good3 = recs[3]
    bad = bytearray(recs[3])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[3] = bytes(bad)
    n, skip, qmax, qmin = len(recs), 2, 100, 20
    ids = [ob.synth_read_id(i) for i in range(n)]
    ids = [i if isinstance(i, bytes) else i.encode() for i in ids]
    levels = rng.normal(500.0, 110.0, 400).astype(np.float32)
    ref = quant_ref(levels)
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("# expected levels\n" + "".join("%.9g\n" % v for v in levels))
    # the restatement: events_dev and queries_dev on the decoded batch, path_ref on each query
    dec = gpu.press.decode_to_device(recs)
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:n, 0].contiguous()
    ev_rows, first = gpu.events.events_dev(dec, DNA, "raw")
    q, ql, qst = gpu.map.queries_dev(ev_rows, first, fst, skip, qmax, qmin)
    h_ev, h_first = ev_rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    qm, qlens, qst = q.cpu().numpy(), ql.cpu().numpy().tolist(), qst.cpu().numpy()
    assert qlens[2] == 0 and qst[2] == QUERY_SHORT and qlens[3] == 0 and qst[3] not in (0, QUERY_SHORT) and min(qlens[i] for i in (0, 1, 4, 5)) >= qmin
    assert qlens[0] == qmax and qlens[1] < qmax
    wlo, whi, wrows = _want(qm, qlens, ref, qmax)
    wst = [int(s) for s in qst]
    wev = np.zeros((n, qmax), dtype=EVENT)
    for i in range(n):
        wev[i, :qlens[i]] = h_ev[h_first[i] + skip:h_first[i] + skip + qlens[i]]
    kw = dict(skip=skip, qmax=qmax, qmin=qmin)
    # align_dev
    rows, lo, hi, st = al.align_dev(dec, ref, **kw)
    assert rows.tolist() == wrows.tolist() and np.array_equal(lo, wlo) and np.array_equal(hi, whi) and st.tolist() == wst
    # read_align
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        al.read_align(recs, ref, **kw)
    rows, lo, hi, ev, st = al.read_align(recs, ref, raise_on_error=False, **kw)
    assert rows.dtype == MAP_ROW and rows.tolist() == wrows.tolist() and np.array_equal(lo, wlo) and np.array_equal(hi, whi) and st.tolist() == wst
    assert ev.dtype == EVENT and ev.tobytes() == wev.tobytes()
    rows2, lo2, hi2, ev2, st2 = al.read_align(recs[:3] + [good3] + recs[4:], ref, **kw)
    keep = [0, 1, 2, 4, 5]
    assert st2[3] == 0 and rows2[3]["qlen"] == qmax and np.array_equal(lo2[keep], wlo[keep]) and rows2[keep].tolist() == wrows[keep].tolist()
    # the tool: exit 1, the corrupt read named, the other reads' lines
    synth_file(tmp_path / "reads.blow5", recs)
    args = ["--skip", str(skip), "--events", str(qmax), "--min-events", str(qmin), str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([al.S5ALIGN, "-K", "4"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and ids[3] in p.stderr and b"short" in p.stderr, p.stderr
    want_lines = []
    for i in keep:
        if qlens[i] == 0:
            want_lines.append(ids[i] + b"\t*\t*\t*\t*\t*\t*\n")
        for k in range(qlens[i]):
            e = wev[i, k]
            want_lines.append(b"%s\t%d\t%d\t%d\t%s\t%d\t%d\n" % (ids[i], skip + k, e["start"], e["start"] + e["length"], b"%.6g" % float(e["mean"]), wlo[i, k], whi[i, k]))
    assert p.stdout == b"".join(want_lines)
    # file_align parses them back
    fids, frows = al.file_align(tmp_path / "reads.blow5", ref_txt, batch=4, raise_on_corrupt=False, **kw)
    assert fids == [ids[i] for i in keep]
    for i, r in zip(keep, frows):
        assert r["event"].tolist() == list(range(skip, skip + qlens[i])) and r["lo"].tolist() == wlo[i, :qlens[i]].tolist()
        assert r["hi"].tolist() == whi[i, :qlens[i]].tolist() and r["sample_start"].tolist() == wev[i, :qlens[i]]["start"].tolist()
        assert r["sample_end"].tolist() == (wev[i, :qlens[i]]["start"] + wev[i, :qlens[i]]["length"]).tolist()
    with pytest.raises(gpu.lib.S5GpuError):
        al.file_align(tmp_path / "reads.blow5", ref_txt, **kw)
    # --max-span 1: no read of these has a path of one column
    assert ((wrows["end"] - wrows["start"])[[0, 1, 4, 5]] > 0).all()
    p = subprocess.run([al.S5ALIGN, "--max-span", "1"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and p.stdout == b"".join(ids[i] + b"\t*\t*\t*\t*\t*\t*\n" for i in keep) and b"wide" in p.stderr
    assert subprocess.run([al.S5ALIGN], capture_output=True).returncode == 2
    assert subprocess.run([al.S5ALIGN, "--max-span", "0"] + args, capture_output=True).returncode == 2
