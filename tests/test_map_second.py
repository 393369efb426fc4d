"""map, the second-best hit and a mapping quality, and a reference made from sequences and a k-mer model (docs/codecs.md §4.19;
slow5tools_amd/csrc/dtw_dev.h `lane_second`, dtw_kernels.hip `k_sdtw2`, refseq.c).

The oracle is numpy, kept in this file: the last row of §4.16's matrix by its recurrence, the direct definition of cost2 / end2 / mapq over
that row, and the level, segment and wall rules of a reference.  Everything is integer from the quantiser onward, so the library is held
to it exactly.  The restatement of the best hit (cost, start, end) and of the quantiser is that of tests/dtw_ref.py.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from blow5_fixture import Blow5, golden
from chain_common import DNA, EVENT, GUARD, MAP_ROW, NO_COST, QUERY_SHORT, ROOT, host_build
from chain_common import gpu  # noqa: F401
from dtw_ref import QLENS, RS, _g_of, last_lane_batch, map_lines, quant_ref, sdtw_ref
from dtw_ref import map_ref, mixed_batches  # noqa: F401

MAP_SECOND = np.dtype([("cost2", "<u4"), ("end2", "<i4"), ("mapq", "<u4"), ("zero", "<u4")])
NONE2 = (NO_COST, -1, 0, 0)
RNA = (7, 14, 2.5, 9.0, 1.0)                                               # s5map --rna's event parameters
WALL = -32768


# ---------------------------------------------------------------------------------------------------------------- the restatement

def last_rows(q, r):
    """L[j] = D[Q - 1][j] of §4.16 for a batch q[B, Q] (or one query q[Q]) against r[R], int32 (a cell is < 2^26), along anti-diagonals"""
    q = np.asarray(q).astype(np.int32)
    one = q.ndim == 1
    if one:
        q = q[None, :]
    r = np.asarray(r).astype(np.int32)
    B, Q = q.shape
    R = len(r)
    D = np.full((B, Q + 1, R + 1), 1 << 30, dtype=np.int32)
    D[:, 0, :] = 0
    for k in range(Q + R - 1):
        i = np.arange(max(0, k - R + 1), min(Q - 1, k) + 1)
        j = k - i
        D[:, i + 1, j + 1] = np.abs(q[:, i] - r[j][None, :]) + np.minimum(np.minimum(D[:, i, j], D[:, i, j + 1]), D[:, i + 1, j])
    L = D[:, Q, 1:].astype(np.int64)
    return L[0] if one else L


def second_ref(L, bshift):
    """(cost2, end2, mapq, 0) by the definition: the least L[j] over the columns whose block differs from end's by at least 2, the smallest
    such j; mapq = 60 (cost2 - cost) / cost2 in integers, 0 without a runner-up or with one of cost 0"""
    L = np.asarray(L, dtype=np.int64)
    end = int(np.argmin(L))
    blk = np.arange(len(L)) >> bshift
    ok = np.abs(blk - blk[end]) >= 2
    if not ok.any():
        return NONE2
    end2 = int(np.argmin(np.where(ok, L, np.int64(1) << 40)))
    cost, cost2 = int(L[end]), int(L[end2])
    return (cost2, end2, 0 if cost2 == 0 else (60 * (cost2 - cost)) // cost2, 0)


def seconds_ref(queries, qlens, r, bshift):
    out = np.zeros(len(qlens), dtype=MAP_SECOND)
    for i, n in enumerate(qlens):
        out[i] = NONE2 if n == 0 else second_ref(last_rows(np.asarray(queries[i])[:n], r), bshift)
    return out


def list_of_four(L, bshift):
    """the one-pass form of the issue: the four least block minima (each with its smallest column), sorted by value, the earlier block first
    among equals; the runner-up is the first whose block is not within 1 of the first one's"""
    L = np.asarray(L, dtype=np.int64)
    mins = []
    for b0 in range(0, len(L), 1 << bshift):
        blk = L[b0:b0 + (1 << bshift)]
        mins.append((int(blk.min()), b0 + int(np.argmin(blk))))
    mins = sorted(mins, key=lambda t: t[0])[:4]                            # (sorted is stable: the earlier block stays first)
    for v, c in mins[1:]:
        if abs((c >> bshift) - (mins[0][1] >> bshift)) >= 2:
            return (v, c, 0 if v == 0 else (60 * (v - mins[0][0])) // v, 0)
    return NONE2


COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def levels_ref(seq, model, k):
    """the L - k + 1 levels of a sequence: the model's by k-mer rank (A, C, G, T = 0 .. 3, the first base most significant), the table's mean
    (the float64 sum in rank order, divided, rounded to float32) for a k-mer that holds any other letter"""
    s = seq.upper().replace("U", "T")
    mean = np.float32(np.cumsum(np.asarray(model, dtype=np.float32).astype(np.float64))[-1] / np.float64(len(model)))
    out = np.zeros(max(len(s) - k + 1, 0), dtype=np.float32)
    for p in range(len(out)):
        km = s[p:p + k]
        out[p] = model[int("".join(str("ACGT".index(c)) for c in km), 4)] if all(c in "ACGT" for c in km) else mean
    return out


def revcomp(seq):
    return "".join(COMP.get(c, "N") for c in reversed(seq.upper().replace("U", "T")))


def refseq_ref(contigs, model, k, strands=2, rna=False, scale=32.0, clip=127):
    """-> (ref int16, segments [(contig, strand, offset, Lk, reversed)], W): the segments in their order, quantised together, walls between"""
    segs, lev = [], []
    for ci, (name, seq) in enumerate(contigs):
        if len(seq) < k:
            continue
        f = levels_ref(seq, model, k)
        if rna:
            segs.append((ci, "+", len(f), True)); lev.append(f[::-1])
            continue
        segs.append((ci, "+", len(f), False)); lev.append(f)
        if strands == 2:
            segs.append((ci, "-", len(f), True)); lev.append(levels_ref(revcomp(seq), model, k))
    W = (2048 * clip) // (32768 - clip) + 1
    q = quant_ref(np.concatenate(lev), scale, clip)
    ref, out, at = [], [], 0
    for n, (ci, strand, Lk, rev) in enumerate(segs):
        if n:
            ref.append(np.full(W, WALL, dtype=np.int16))
        out.append((ci, strand, sum(len(x) for x in ref), Lk, rev))
        ref.append(q[at:at + Lk])
        at += Lk
    return np.concatenate(ref), out, W


def synth_model(k, seed=5):
    """a synthetic k-mer table: 4^k levels around 90 pA, no two the same"""
    rng = np.random.default_rng(seed)
    return (60.0 + rng.permutation(4 ** k) * (60.0 / 4 ** k) + rng.uniform(0.0, 0.2, 4 ** k)).astype(np.float32)


def write_model(path, model, k, header=True, skip=(), twice=()):
    with open(path, "w") as fh:
        if header:
            fh.write("# a synthetic model\nkmer\tlevel_mean\tlevel_stdv\n")
        for rank in range(4 ** k):
            km = "".join("ACGT"[(rank >> (2 * (k - 1 - b))) & 3] for b in range(k))
            if rank in skip:
                continue
            fh.write("%s\t%.9g\t1.5\n" % (km, model[rank]) if rank % 2 else "%s   %.9g\n" % (km, model[rank]))
            if rank in twice:
                fh.write("%s\t%.9g\n" % (km, model[rank]))


def random_seq(rng, n):
    return "".join("ACGT"[v] for v in rng.integers(0, 4, n))


# ---------------------------------------------------------------------------------------------------------------- not gpu

CALLS = {"s5gpu_sdtw2_dev": 11, "s5gpu_map2_batch": 13, "s5gpu_kmer_model_load": 3, "s5gpu_kmer_model_free": 1, "s5gpu_refseq_build": 10,
         "s5gpu_refseq_open": 6, "s5gpu_refseq_ref": 2, "s5gpu_refseq_n_segments": 1, "s5gpu_refseq_segment": 3, "s5gpu_refseq_n_contigs": 1,
         "s5gpu_refseq_contig": 5, "s5gpu_refseq_params": 4, "s5gpu_refseq_locate": 3, "s5gpu_refseq_close": 1}


def test_library_exports_the_new_calls():
    from slow5tools_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert {s: len(getattr(L, s).argtypes) for s in CALLS} == CALLS


def test_second_layouts_match_header(tmp_path):
    from slow5tools_amd import _lib
    from slow5tools_amd import map as smap

    sec, seg, loc = ["cost2", "end2", "mapq", "zero"], ["contig", "strand", "offset", "Lk", "reversed", "zero", "name"], ["contig", "strand", "pos", "segment"]
    src = tmp_path / "ly.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){printf("%zu", sizeof(s5gpu_map_second_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_map_second_t, %s));\n' % m for m in sec)
                   + 'printf(" %zu", sizeof(s5gpu_refseq_segment_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_refseq_segment_t, %s));\n' % m for m in seg)
                   + 'printf(" %zu", sizeof(s5gpu_refseq_loc_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_refseq_loc_t, %s));\n' % m for m in loc)
                   + 'printf(" %d\\n", S5GPU_REFSEQ_WALL);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "ly")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ly")], text=True).split()]
    D, Sg, Lc = smap.MAP_SECOND, _lib.RefSeqSegment, _lib.RefSeqLoc
    assert got == ([D.itemsize] + [D.fields[m][1] for m in sec] + [C.sizeof(Sg)] + [getattr(Sg, m).offset for m in seg]
                   + [C.sizeof(Lc)] + [getattr(Lc, m).offset for m in loc] + [_lib.REFSEQ_WALL])
    assert D == MAP_SECOND and D.itemsize == 16


def test_the_list_of_four_equals_the_definition():
    """the one-pass form against the direct definition on 300 random last rows, ties included"""
    rng = np.random.default_rng(77)
    some = 0
    for t in range(300):
        R = int(rng.integers(1, 700))
        L = rng.integers(0, 4 if t % 2 else 5000, R)
        for b in (6, 7):
            want = second_ref(L, b)
            assert list_of_four(L, b) == want, (t, R, b)
            some += want != NONE2
    assert 100 < some < 600


SECOND_HOST = r'''
// lane_second, second_flush and second_row of dtw_dev.h on the CPU beside lane_step and lane_best: 64 lanes in lockstep, the lane exchange as in
// tests/test_map.py; the flush is taken by every lane at the step at which the lane of row Q - 1 has done the last column of a block, and
// once more after the walk.  out.bin gets, per case, the row and the second row without and with want_start.
#define S5_DTW_HOST
#include "dtw_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace dtwk;
static void shift_up1(const uint32_t *v, uint32_t fill, uint32_t *out) { for (int l = 63; l >= 1; l--) out[l] = v[l - 1]; out[0] = fill; }

template <int G, bool WS, int KB>
static void run(const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R, uint32_t bshift, U4 *out) {
    std::vector<Lane<G, WS> > L(64);
    std::vector<Second> S(64);
    uint32_t rcur[64], v[64], r[64], up[64], sup[64];
    for (uint32_t l = 0; l < 64; l++) {
        lane_init(L[l], l == 0);
        second_init(S[l]);
        rcur[l] = 0; sup[l] = 0xFFFFFFFFu;
        for (int k = 0; k < G; k++) { const uint32_t row = l * G + k; L[l].q[k] = biased(row < Q ? q[row] : (int16_t)0); }
    }
    const uint32_t last = (Q - 1) / G, steps = R + last;
    if ((int)(Q - 1 - last * G) != KB) abort();
    for (uint32_t t = 0; t < steps; t++) {
        const uint32_t r0 = biased(t < R ? ref[t] : (int16_t)0);
        shift_up1(rcur, r0, r);
        for (int l = 0; l < 64; l++) { rcur[l] = r[l]; v[l] = L[l].d[G - 1]; }
        shift_up1(v, 0u, up);
        if (WS) { for (int l = 0; l < 64; l++) v[l] = (uint32_t)L[l].s[G - 1]; shift_up1(v, t + 1, sup); }
        for (uint32_t l = 0; l < 64; l++) {
            lane_step(L[l], r[l], up[l], (int32_t)sup[l]);
            lane_best<G, WS, KB>(L[l], t - l, R);
            lane_second<G, WS, KB>(L[l], S[l], t - l, R);
        }
        if (second_block_ends(t - last, bshift))
            for (uint32_t l = 0; l < 64; l++) second_flush(S[l]);
    }
    for (uint32_t l = 0; l < 64; l++) second_flush(S[l]);
    out[0] = result_row(L[last].best, Q, WS ? L[last].best_start : -1, L[last].best_end);
    out[1] = second_row(S[last], bshift);
}
template <int G, int KB = 0>
struct Pick {
    static void go(int kb, const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R, uint32_t bshift, U4 *out) {
        if (kb == KB) { run<G, false, KB>(q, Q, ref, R, bshift, out); run<G, true, KB>(q, Q, ref, R, bshift, out + 2); }
        else if constexpr (KB + 1 < G) Pick<G, KB + 1>::go(kb, q, Q, ref, R, bshift, out);
    }
};
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (argc != 3 || !f || !o) return 1;
    for (;;) {
        uint32_t Q, R, G, bshift;
        if (fread(&Q, 4, 1, f) != 1) break;
        if (fread(&R, 4, 1, f) != 1 || fread(&G, 4, 1, f) != 1 || fread(&bshift, 4, 1, f) != 1 || Q < 1 || Q > 64 * G || R < 1) return 1;
        std::vector<int16_t> q(Q), r(R);
        if (fread(q.data(), 2, Q, f) != Q || fread(r.data(), 2, R, f) != R) return 1;
        const int kb = (int)((Q - 1) % G);
        U4 out[4];
        memset(out, 0xEE, sizeof out);
        if (G == 1) Pick<1>::go(kb, q.data(), Q, r.data(), R, bshift, out);
        else if (G == 2) Pick<2>::go(kb, q.data(), Q, r.data(), R, bshift, out);
        else if (G == 4) Pick<4>::go(kb, q.data(), Q, r.data(), R, bshift, out);
        else if (G == 8) Pick<8>::go(kb, q.data(), Q, r.data(), R, bshift, out);
        else if (G == 16) Pick<16>::go(kb, q.data(), Q, r.data(), R, bshift, out);
        else return 1;
        fwrite(out, 16, 4, o);
    }
    return fclose(o) == 0 ? 0 : 1;
}
'''


def test_lane_second_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """lane_second, second_flush and second_row of dtw_dev.h as g++ compiles them, in 64-lane lockstep: every Q and R of the issue at block
    shifts 6 and 7, values of +-127 and of {-1, 0, 1} (ties); references within three blocks (no runner-up unless the best hit is in an outer
    one); a best hit planted in the first block and in the last"""
    rng = np.random.default_rng(19)
    cases = []
    for Q in (1, 63, 64, 65, 130, 1000):
        for R in (1, 63, 64, 65, 129, 500):
            for b in (6, 7):
                cases.append((rng.integers(-127, 128, Q), rng.integers(-127, 128, R), _g_of(Q), b))
                cases.append((rng.integers(-1, 2, Q), rng.integers(-1, 2, R), _g_of(Q), b))
    for b in (6, 7):                                                       # three blocks exactly, and one column more
        for R in (3 << b, (3 << b) + 1):
            cases.append((rng.integers(-127, 128, 40), rng.integers(-127, 128, R), 1, b))
    planted = []
    for Q, R in ((40, 500), (63, 700), (64, 900)):
        q = rng.integers(-127, 128, Q)
        first, lastb = rng.integers(-127, 128, R), rng.integers(-127, 128, R)
        first[:Q], lastb[R - Q:] = q, q
        planted += [(len(cases), 0), (len(cases) + 1, (R - 1) >> 6)]
        cases += [(q, first, _g_of(Q), 6), (q, lastb, _g_of(Q), 6)]
    cases.append((rng.integers(-127, 128, 5), rng.integers(-127, 128, 400), 4, 6))      # a lane height above the smallest
    cases = [(np.asarray(q, dtype=np.int16), np.asarray(r, dtype=np.int16), g, b) for q, r, g, b in cases]
    with open(tmp_path / "in.bin", "wb") as fh:
        for q, r, g, b in cases:
            fh.write(struct.pack("<IIII", len(q), len(r), g, b) + q.tobytes() + r.tobytes())
    exe = host_build(tmp_path, "second_host", SECOND_HOST, ["-O1", "-std=c++17", "-ffp-contract=off"])
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 64 * len(cases)
    none = some = 0
    for n, (q, r, g, b) in enumerate(cases):
        rows = np.frombuffer(raw, MAP_ROW, 4, 64 * n)
        sec = np.frombuffer(raw, MAP_SECOND, 4, 64 * n)
        c, s, e = sdtw_ref(q, r)
        L = last_rows(q, r)
        want = second_ref(L, b)
        assert int(L.min()) == c and int(np.argmin(L)) == e
        assert rows[0].tolist() == (c, len(q), -1, e) and rows[2].tolist() == (c, len(q), s, e), (len(q), len(r), g, b)
        assert sec[1].tolist() == want and sec[3].tolist() == want, (len(q), len(r), g, b, sec[1].tolist(), want)
        if len(r) <= 2 << b:
            assert want == NONE2
        none += want == NONE2
        some += want != NONE2
    assert none > 20 and some > 20
    for n, block in planted:                                               # the best hit in the first and in the last block, a runner-up elsewhere
        q, r, g, b = cases[n]
        c, s, e = sdtw_ref(q, r)
        assert c == 0 and e >> b == block and second_ref(last_rows(q, r), b) != NONE2


def _contigs3():
    rng = np.random.default_rng(41)
    return [("chrA", random_seq(rng, 90)), ("tiny", "AC"), ("chrB extra words", random_seq(rng, 40) + "N" + random_seq(rng, 30)), ("chrC", random_seq(rng, 57).lower())]


def _refseq(contigs, model, **kw):
    from slow5tools_amd import map as smap

    return smap.RefSeq(contigs=[(n.split()[0], s) for n, s in contigs], levels=model, **kw)


def test_model_and_fasta_parsing(tmp_path):
    from slow5tools_amd import _lib
    from slow5tools_amd import map as smap

    L = _lib.lib()
    k, model = 3, synth_model(3)
    write_model(tmp_path / "ok.model", model, k)
    lv, kk = C.POINTER(C.c_float)(), C.c_uint32()
    assert L.s5gpu_kmer_model_load(os.fsencode(tmp_path / "ok.model"), C.byref(lv), C.byref(kk)) == 0 and kk.value == 3
    assert np.array_equal(np.ctypeslib.as_array(lv, (64,)), model)         # %.9g round-trips a float32
    L.s5gpu_kmer_model_free(lv)
    # refused: a k-mer missing, one twice, one of another length, a line without a level, letters outside ACGT, an empty file, no file
    write_model(tmp_path / "missing.model", model, k, skip=(17,))
    write_model(tmp_path / "twice.model", model, k, twice=(5,))
    (tmp_path / "length.model").write_text((tmp_path / "ok.model").read_text() + "ACGT\t80.0\n")
    (tmp_path / "nolevel.model").write_text((tmp_path / "ok.model").read_text().replace("%.9g" % model[9], "abc"))
    (tmp_path / "letters.model").write_text((tmp_path / "ok.model").read_text().replace("ACG", "ANG"))
    (tmp_path / "empty.model").write_text("# nothing\nkmer\tlevel_mean\n")
    for name, rc in (("missing", -5), ("twice", -5), ("length", -5), ("nolevel", -5), ("letters", -5), ("empty", -5), ("absent", -1)):
        lv = C.POINTER(C.c_float)()
        assert L.s5gpu_kmer_model_load(os.fsencode(tmp_path / (name + ".model")), C.byref(lv), C.byref(kk)) == rc, name
        assert not lv
    # FASTA: names up to the first white space, a sequence over several lines, lower case, U as T, N takes the mean, a contig shorter than k
    contigs = _contigs3()
    with open(tmp_path / "ref.fa", "w") as fh:
        for name, seq in contigs:
            s = seq.replace("t", "u") if name == "chrC" else seq
            fh.write(">%s\n" % name + "".join(s[a:a + 25] + "\n" for a in range(0, len(s), 25)) + "\n")
    rs = smap.RefSeq(fasta=tmp_path / "ref.fa", model=tmp_path / "ok.model")
    want, segs, W = refseq_ref(contigs, model, k)
    assert W == 8 == rs.wall and rs.k == 3 and rs.clip == 127
    assert rs.ref.dtype == np.int16 and np.array_equal(rs.ref, want)
    assert rs.contigs == [("chrA", 90, 88), ("tiny", 2, 0), ("chrB", 71, 69), ("chrC", 57, 55)]
    assert rs.segments == [(ci, contigs[ci][0].split()[0], strand, off, Lk) for ci, strand, off, Lk, rev in segs] and len(segs) == 6
    n_mean = int((levels_ref(contigs[2][1], model, k) == levels_ref("ANA", model, k)[0]).sum())
    assert n_mean == 3                                                     # the three k-mers that hold the N
    # the same from memory
    assert np.array_equal(_refseq(contigs, model).ref, want)
    # refused: an empty FASTA, sequence in front of the first name, no contig of k bases, an incomplete model, a missing file
    (tmp_path / "empty.fa").write_text("\n")
    (tmp_path / "headless.fa").write_text("ACGT\n>x\nACGT\n")
    (tmp_path / "short.fa").write_text(">x\nAC\n>y\n\n")
    for fa, mo in (("empty.fa", "ok.model"), ("headless.fa", "ok.model"), ("short.fa", "ok.model"), ("ref.fa", "missing.model"), ("none.fa", "ok.model")):
        with pytest.raises(_lib.S5GpuError):
            smap.RefSeq(fasta=tmp_path / fa, model=tmp_path / mo)


def test_levels_segments_and_walls_equal_the_restatement():
    from slow5tools_amd import _lib

    contigs = _contigs3()
    for k in (1, 3, 5):
        model = synth_model(k, seed=k)
        for kw in (dict(), dict(strands=1), dict(rna=True), dict(rna=True, strands=1), dict(scale=20.0, clip=60)):
            rs = _refseq(contigs, model, **kw)
            want, segs, W = refseq_ref(contigs, model, k, **kw)
            assert np.array_equal(rs.ref, want) and rs.wall == W, (k, kw)
            assert [(c, s, o, l) for c, n, s, o, l in rs.segments] == [(c, s, o, l) for c, s, o, l, rev in segs], (k, kw)
            long_enough = sum(len(s) >= k for n, s in contigs)             # ("tiny" has a segment at k = 1 only)
            assert len(segs) == long_enough * (1 if kw.get("rna") or kw.get("strands") == 1 else 2) and long_enough == (4 if k == 1 else 3)
            # the walls stand between consecutive segments and nowhere else
            is_wall = np.ones(len(want), dtype=bool)
            for c, s, o, l, rev in segs:
                is_wall[o:o + l] = False
            assert is_wall.sum() == W * (len(segs) - 1) and (want[is_wall] == WALL).all() and (np.abs(want[~is_wall].astype(int)) <= kw.get("clip", 127)).all()
    # the reverse strand is the reverse complement's levels: column p' is forward k-mer start Lk - 1 - p', and RNA is the forward levels reversed
    k, model = 3, synth_model(3)
    seq = contigs[0][1]
    f, r = levels_ref(seq, model, k), levels_ref(revcomp(seq), model, k)
    for p in range(len(r)):
        assert r[p] == levels_ref(revcomp(seq[len(f) - 1 - p:len(f) - 1 - p + k]), model, k)[0]
    one = [contigs[0]]
    assert np.array_equal(_refseq(one, model, rna=True).ref, quant_ref(f[::-1]))
    assert np.array_equal(_refseq(one, model, strands=1).ref, quant_ref(f))
    # W = (2048 clip) / (32768 - clip) + 1: 8 at 127; above 64 it is refused, as are k and strands out of range
    assert _refseq(one, model, clip=127).wall == 8 and _refseq(one, model, clip=1).wall == 1 and _refseq(one, model, clip=992).wall == 64
    for kw in (dict(clip=993), dict(clip=32767), dict(clip=0), dict(strands=3), dict(strands=0), dict(scale=0.0)):
        with pytest.raises(_lib.S5GpuError):
            _refseq(one, model, **kw)
    with pytest.raises(_lib.S5GpuError):
        _refseq([("x", "AC")], model)
    with pytest.raises(ValueError):
        _refseq(one, model[:63])


def test_locate_is_the_inverse_of_the_layout():
    contigs, k, model = _contigs3(), 3, synth_model(3)
    for kw in (dict(), dict(strands=1), dict(rna=True)):
        rs = _refseq(contigs, model, **kw)
        want, segs, W = refseq_ref(contigs, model, k, **kw)
        expect = [(-1, "wall", -1)] * len(want)
        for c, s, o, l, rev in segs:
            for p in range(l):
                expect[o + p] = (c, s, l - 1 - p if rev else p)
        assert rs.locate(np.arange(len(want))) == expect
        assert sum(e[0] < 0 for e in expect) == W * (len(segs) - 1)
        with pytest.raises(Exception):
            rs.locate([len(want)])
        # spans: a row's (start, end) -> forward coordinates, lo <= hi; a span over a wall is no span
        c, s, o, l, rev = segs[-1]
        rows = np.array([(5, 10, o + 3, o + 12), (NO_COST, 0, -1, -1), (5, 10, segs[0][2] + 2, o + 1)], dtype=MAP_ROW)
        lo, hi = (l - 1 - 12, l - 1 - 3) if rev else (3, 12)
        assert rs.spans(rows) == [(c, s, lo, hi), None, None]


def _three_segments(rng, lens):
    segs = [rng.integers(-127, 128, n).astype(np.int16) for n in lens]
    wall = np.full(8, WALL, dtype=np.int16)
    ref = np.concatenate([segs[0], wall, segs[1], wall, segs[2]])
    offs = [0, lens[0] + 8, lens[0] + lens[1] + 16]
    return ref, segs, offs


def test_the_wall_property_on_the_restatement():
    """On references of three segments with walls of 8 columns of -32768 between them: the best hit's span lies in one segment, and its cost
    is the least of the three costs of the query against the segments alone.  30 random draws, and 30 whose query is the end of one segment
    followed by the start of the next: a path across the wall would cost nothing but the wall."""
    rng = np.random.default_rng(61)
    for t in range(60):
        lens = [int(v) for v in rng.integers(30, 80, 3)]
        ref, segs, offs = _three_segments(rng, lens)
        if t < 30:
            q = rng.integers(-127, 128, int(rng.integers(1, 70))).astype(np.int16)
        else:
            a, n = int(rng.integers(0, 2)), int(rng.integers(5, 25))
            q = np.concatenate([segs[a][-n:], segs[a + 1][:n]])
        c, s, e = sdtw_ref(q, ref)
        inside = [o <= s and e < o + n for o, n in zip(offs, lens)]
        assert sum(inside) == 1, (t, s, e)
        alone = [sdtw_ref(q, sg)[0] for sg in segs]
        assert c == min(alone) and alone[inside.index(True)] == c, t
        if t >= 30:
            assert c > 0                                                   # (the crossing it was tempted with would have cost 0 but for the wall)


# ---------------------------------------------------------------------------------------------------------------- gpu

def _run_sdtw2(env, qm, qlens, ref, want_start, bshift=6, compare=True):
    """s5gpu_sdtw2_dev on a query matrix with guard rows around both outputs -> (MAP_ROW array, MAP_SECOND array); out_rows is held to what
    s5gpu_sdtw_dev writes for the same arguments, bit for bit"""
    torch, L = env.torch, env.L
    n = len(qlens)
    d_q = torch.from_numpy(np.ascontiguousarray(qm)).to("cuda")
    d_ql = torch.from_numpy(np.asarray(qlens, dtype=np.int32)).to("cuda")
    d_r = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16)).to("cuda")
    d_out = torch.full(((n + 2) * 4,), GUARD, dtype=torch.int32, device="cuda")
    d_out2 = torch.full(((n + 2) * 4,), GUARD, dtype=torch.int32, device="cuda")
    d_old = torch.full((n * 4,), GUARD, dtype=torch.int32, device="cuda")
    env.lib.check(L.s5gpu_sdtw2_dev(n, d_q.data_ptr(), qm.shape[1], d_ql.data_ptr(), d_r.data_ptr(), len(ref), int(want_start), bshift,
                                    d_out.data_ptr() + 16, d_out2.data_ptr() + 16, None), "s5gpu_sdtw2_dev")
    env.lib.check(L.s5gpu_sdtw_dev(n, d_q.data_ptr(), qm.shape[1], d_ql.data_ptr(), d_r.data_ptr(), len(ref), int(want_start), d_old.data_ptr(), None),
                  "s5gpu_sdtw_dev")
    torch.cuda.synchronize()
    out, out2 = d_out.cpu().numpy(), d_out2.cpu().numpy()
    for o in (out, out2):
        assert (o[:4] == GUARD).all() and (o[-4:] == GUARD).all(), "a guard row around an output was written"
    assert np.array_equal(d_q.cpu().numpy(), qm) and np.array_equal(d_r.cpu().numpy(), np.asarray(ref, dtype=np.int16))
    if compare:
        assert np.array_equal(out[4:-4], d_old.cpu().numpy()), "out_rows differs from s5gpu_sdtw_dev's"
    return out[4:-4].view(MAP_ROW).copy(), out2[4:-4].view(MAP_SECOND).copy()


def _check_second(got, want, what):
    for col in ("cost2", "end2", "mapq", "zero"):
        bad = np.nonzero(got[col] != want[col])[0]
        assert len(bad) == 0, (what, col, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lo,hi", [("pm127", -127, 127), ("ties", -1, 1)])
@pytest.mark.parametrize("R", RS)
def test_sdtw2_is_exact_on_the_mixed_batch(gpu, mixed_batches, R, kind, lo, hi):
    rng = np.random.default_rng(300 + R)
    qm, ref = mixed_batches[kind], rng.integers(lo, hi + 1, R).astype(np.int16)
    want = seconds_ref(qm, QLENS, ref, 6)
    assert want[0].tolist() == NONE2
    if R <= 128:
        assert (want["end2"] == -1).all()
    for ws in (False, True):
        rows, sec = _run_sdtw2(gpu, qm, QLENS, ref, ws)
        _check_second(sec, want, (R, kind, ws))
        assert rows["qlen"].tolist() == QLENS and (rows["start"][1:] >= 0).all() == ws
    if R == 500:
        assert (want["end2"][1:] >= 0).all() and (want["mapq"] <= 60).all()
        assert (np.abs((want["end2"][1:] >> 6) - (rows["end"][1:] >> 6)) >= 2).all()
        got7 = _run_sdtw2(gpu, qm, QLENS, ref, False, bshift=7)[1]
        _check_second(got7, seconds_ref(qm, QLENS, ref, 7), (R, kind, "bshift 7"))


@pytest.mark.gpu
def test_sdtw2_every_row_of_the_last_lane(gpu):
    qm, ql = last_lane_batch()
    ref = np.random.default_rng(43).integers(-127, 128, 300).astype(np.int16)
    last = [last_rows(qm[i, :n], ref) for i, n in enumerate(ql)]
    want = np.array([second_ref(L, 6) for L in last], dtype=MAP_SECOND)
    assert (want["end2"] >= 0).all() and (want["cost2"] < 2 ** 26).all()                                       # every read has a runner-up
    for ws in (False, True):
        rows, sec = _run_sdtw2(gpu, qm, ql, ref, ws)
        _check_second(sec, want, ("every row of the last lane", ws))
        assert rows["qlen"].tolist() == ql and (rows["start"] >= 0).all() == ws
        assert rows["cost"].tolist() == [int(L.min()) for L in last] and rows["end"].tolist() == [int(L.argmin()) for L in last]


@pytest.mark.gpu
def test_sdtw2_many_waves_and_workgroups(gpu):
    rng = np.random.default_rng(8)
    qm, ref = rng.integers(-127, 128, (1000, 48)).astype(np.int16), rng.integers(-127, 128, 333).astype(np.int16)
    L = last_rows(qm, ref)
    want = np.array([second_ref(L[i], 6) for i in range(1000)], dtype=MAP_SECOND)
    rows, sec = _run_sdtw2(gpu, qm, [48] * 1000, ref, True)
    _check_second(sec, want, "n = 1000")
    assert np.array_equal(rows["cost"], L.min(axis=1)) and np.array_equal(rows["end"], L.argmin(axis=1))
    assert (want["end2"] >= 0).all() and len(set(want["end2"].tolist())) > 50 and len(set(want["mapq"].tolist())) > 5


@pytest.mark.gpu
def test_sdtw2_full_int16_range_at_the_overflow_bound(gpu):
    rng = np.random.default_rng(6)
    qm = np.zeros((3, 1024), dtype=np.int16)
    qm[0], qm[1], qm[2, :1000] = 32767, rng.integers(-32768, 32768, 1024), rng.integers(-32768, 32768, 1000)
    ql = [1024, 1024, 1000]
    for ref in (np.full(300, -32768, dtype=np.int16), rng.integers(-32768, 32768, 321).astype(np.int16)):
        want = seconds_ref(qm, ql, ref, 6)
        rows, sec = _run_sdtw2(gpu, qm, ql, ref, True)
        _check_second(sec, want, len(ref))
    # every cell of the last row at 65535 * 1024: the runner-up is the first column two blocks on, at the same cost, and 60 * 0 / cost2 = 0
    assert seconds_ref(qm[:1], ql[:1], np.full(300, -32768, dtype=np.int16), 6)[0].tolist() == (65535 * 1024, 128, 0, 0)


def _planted(rng, copies):
    """a reference of 1200 levels, neighbours at least 20 apart; the 50 levels from column 100 stand again from every column of `copies`;
    the query is that run with every level but the first and the last held 1 to 3 times"""
    lv = [int(rng.integers(-100, 101))]
    while len(lv) < 1200:
        v = int(rng.integers(-100, 101))
        if abs(v - lv[-1]) >= 20:
            lv.append(v)
    ref = np.array(lv, dtype=np.int16)
    for at in copies:
        ref[at:at + 50] = ref[100:150]
    rep = rng.integers(1, 4, 50)
    rep[0] = rep[-1] = 1
    return ref, np.repeat(ref[100:150], rep).astype(np.int16)


@pytest.mark.gpu
def test_planted_hits(gpu):
    rng = np.random.default_rng(15)
    # twice, the copies 9 blocks apart: the runner-up is the second copy at the same cost, and the quality is 0
    ref, q = _planted(rng, [700])
    qm = q[None, :].copy()
    rows, sec = _run_sdtw2(gpu, qm, [len(q)], ref, True)
    assert rows[0].tolist() == (0, len(q), 100, 149) and sec[0].tolist() == (0, 749, 0, 0)
    assert seconds_ref(qm, [len(q)], ref, 6)[0].tolist() == (0, 749, 0, 0)
    # once: a runner-up there is, far worse, and the quality is high
    ref, q = _planted(rng, [])
    qm = q[None, :].copy()
    rows, sec = _run_sdtw2(gpu, qm, [len(q)], ref, True)
    want = seconds_ref(qm, [len(q)], ref, 6)[0]
    assert rows[0].tolist() == (0, len(q), 100, 149) and sec[0].tolist() == want.tolist()
    assert sec[0]["mapq"] == 60 and sec[0]["cost2"] > 0 and abs((int(sec[0]["end2"]) >> 6) - (149 >> 6)) >= 2
    # the python call returns the same
    torch = gpu.torch
    o, o2 = gpu.map.sdtw2_dev(torch.from_numpy(qm).to("cuda"), torch.tensor([len(q)], dtype=torch.int32, device="cuda"), torch.from_numpy(ref).to("cuda"),
                              want_start=True, bshift=6)
    assert o.is_cuda and o2.is_cuda and tuple(o2.shape) == (1, 4) and o2.dtype == torch.int32
    assert o.cpu().numpy().view(MAP_ROW).reshape(-1)[0] == rows[0] and o2.cpu().numpy().view(MAP_SECOND).reshape(-1)[0] == sec[0]
    assert gpu.map.default_bshift(250) == 8 and gpu.map.default_bshift(64) == 6 and gpu.map.default_bshift(65) == 7 and gpu.map.default_bshift(1024) == 10


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    d = tmp_path_factory.mktemp("refseq")
    rng = np.random.default_rng(23)
    contigs = [("ctgA", random_seq(rng, 400)), ("ctgB", random_seq(rng, 500))]
    k, model = 3, synth_model(3)
    write_model(d / "k3.model", model, k)
    with open(d / "two.fa", "w") as fh:
        for name, seq in contigs:
            fh.write(">%s some words\n" % name + "".join(seq[a:a + 60] + "\n" for a in range(0, len(seq), 60)))
    env = type("Env", (), {})()
    env.dir, env.contigs, env.k, env.model, env.fasta, env.model_path = d, contigs, k, model, d / "two.fa", d / "k3.model"
    env.ref, env.segs, env.W = refseq_ref(contigs, model, k)
    return env


@pytest.mark.gpu
def test_both_strands_are_found_and_located(gpu, two_contigs):
    torch, t = gpu.torch, two_contigs
    rs = gpu.map.RefSeq(fasta=t.fasta, model=t.model_path)
    assert np.array_equal(rs.ref, t.ref) and len(rs.segments) == 4
    fwd_a, rev_b = t.segs[0], t.segs[3]
    assert (fwd_a[0], fwd_a[1], rev_b[0], rev_b[1]) == (0, "+", 1, "-")
    cuts = [(fwd_a, 37, 60), (rev_b, 301, 60), (rev_b, 0, 64), (fwd_a, fwd_a[3] - 50, 50)]
    qm = np.zeros((len(cuts), 64), dtype=np.int16)
    for i, ((c, s, o, l, rev), a, n) in enumerate(cuts):
        qm[i, :n] = t.ref[o + a:o + a + n]
    ql = [n for seg, a, n in cuts]
    rows, sec = gpu.map.sdtw2_dev(torch.from_numpy(qm).to("cuda"), torch.tensor(ql, dtype=torch.int32, device="cuda"), torch.from_numpy(rs.ref).to("cuda"),
                                  want_start=True)
    rows, sec = rows.cpu().numpy().view(MAP_ROW).reshape(-1), sec.cpu().numpy().view(MAP_SECOND).reshape(-1)
    assert [(n,) + sdtw_ref(qm[i, :n], t.ref) for i, n in enumerate(ql)] == [(n, 0, o + a, o + a + n - 1) for (c, s, o, l, rev), a, n in cuts]
    assert rows.tolist() == [(0, n, o + a, o + a + n - 1) for (c, s, o, l, rev), a, n in cuts]
    want_spans = [(c, s, (l - 1 - (a + n - 1), l - 1 - a) if rev else (a, a + n - 1)) for (c, s, o, l, rev), a, n in cuts]
    assert rs.spans(rows) == [(c, s, lo, hi) for c, s, (lo, hi) in want_spans]
    assert [sp[1] for sp in rs.spans(rows)] == ["+", "-", "-", "+"] and all(sp[2] <= sp[3] for sp in rs.spans(rows))
    _check_second(sec, seconds_ref(qm, ql, t.ref, 6), "two contigs")
    assert (sec["mapq"] == 60).all()
    # the reverse-strand hit names the bases it came from: the bases of k-mer starts pos_lo .. pos_hi of the forward strand,
    # reverse-complemented, have the levels the query was cut from
    c, s, lo, hi = rs.spans(rows)[1]
    piece = t.contigs[c][1][lo:hi + t.k]
    assert np.array_equal(levels_ref(revcomp(piece), t.model, t.k), levels_ref(revcomp(t.contigs[1][1]), t.model, t.k)[301:361])


def _map2_want(gpu, dec, n, ref, skip, qmax, qmin, want_start, bshift, event_params=DNA):
    """events_dev + quant_ref + the restatement on the host -> (rows, second, status)"""
    rows, first = gpu.events.events_dev(dec, event_params, "raw")
    h, fi = rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    f = dec.t_fields.cpu().numpy().view(gpu.lib.REC_FIELDS)[:n]
    want, want2, st = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=MAP_SECOND), np.zeros(n, dtype=np.int32)
    for i in range(n):
        ev = h[fi[i]:fi[i + 1]]
        m = min(qmax, max(len(ev) - skip, 0))
        if f["status"][i] != 0 or m < qmin:
            want[i], want2[i], st[i] = (NO_COST, 0, -1, -1), NONE2, (f["status"][i] if f["status"][i] != 0 else QUERY_SHORT)
            continue
        q = quant_ref(ev["mean"][skip:skip + m])
        c, s, e = sdtw_ref(q, ref)
        want[i], want2[i] = (c, m, s if want_start else -1, e), second_ref(last_rows(q, ref), bshift)
    return want, want2, st


@pytest.mark.gpu
def test_read_map2_and_map2_dev_on_a_golden_file(gpu, map_ref):
    f = Blow5(golden("exp_1_lossless.blow5"))
    n = len(f.records)
    dec = gpu.press.decode_to_device(f.records, f.rec_method, f.sig_method, no_payload=gpu.press.no_payload_methods(f.rec_method, f.sig_method))
    for skip, qmax, qmin, ws, bshift, b in ((0, 250, 50, True, None, 8), (5, 100, 100, False, 6, 6)):
        want, want2, wst = _map2_want(gpu, dec, n, map_ref, skip, qmax, qmin, ws, b)
        assert (want["qlen"] == qmax).all() and (want2["end2"] >= 0).all() and (want2["cost2"] >= want["cost"]).all()
        got, got2, st = gpu.map.read_map2(f.records, map_ref, f.rec_method, f.sig_method, skip=skip, qmax=qmax, qmin=qmin, want_start=ws, bshift=bshift)
        assert got.dtype == MAP_ROW and got2.dtype == MAP_SECOND
        assert got.tolist() == want.tolist() and got2.tolist() == want2.tolist() and st.tolist() == wst.tolist(), ("read_map2", skip, qmax)
        got, got2, st = gpu.map.map2_dev(dec, map_ref, skip=skip, qmax=qmax, qmin=qmin, want_start=ws, bshift=bshift)
        assert got.tolist() == want.tolist() and got2.tolist() == want2.tolist() and st.tolist() == wst.tolist(), ("map2_dev", skip, qmax)
        old, ost = gpu.map.read_map(f.records, map_ref, f.rec_method, f.sig_method, skip=skip, qmax=qmax, qmin=qmin, want_start=ws)
        assert old.tolist() == want.tolist() and ost.tolist() == wst.tolist()
    got, got2, st = gpu.map.read_map2(f.records, map_ref, f.rec_method, f.sig_method, skip=1 << 30, qmax=10, qmin=1)
    assert got.tolist() == [(NO_COST, 0, -1, -1)] * n and got2.tolist() == [NONE2] * n and st.tolist() == [QUERY_SHORT] * n


@pytest.mark.gpu
def test_map2_batch_with_a_corrupt_record(gpu, map_ref):
    m = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    recs = list(m.records)
    good, good2, st0 = gpu.map.read_map2(recs, map_ref, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True)
    assert not st0.any() and (good["qlen"] == 64).all() and (good2["end2"] >= 0).all()
    bad = bytearray(recs[1])
    bad[-1] ^= 0x5A
    recs[1] = bytes(bad)
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        gpu.map.read_map2(recs, map_ref, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True)
    got, got2, st = gpu.map.read_map2(recs, map_ref, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True, raise_on_error=False)
    assert st[1] not in (0, QUERY_SHORT) and not st[0] and not st[2:].any()
    assert got[1].tolist() == (NO_COST, 0, -1, -1) and got2[1].tolist() == NONE2
    assert got[0] == good[0] and np.array_equal(got[2:], good[2:]) and got2[0] == good2[0] and np.array_equal(got2[2:], good2[2:])


def _lines2(ids, rows, sec, want_start):
    out = []
    for line, r, s in zip(map_lines(ids, rows, want_start).split(b"\n"), rows, sec):
        tail = b"\t*\t*\t*" if r["qlen"] == 0 else b"\t*\t*\t%d" % s["mapq"] if s["end2"] < 0 else b"\t%d\t%d\t%d" % (s["cost2"], s["end2"], s["mapq"])
        out.append(line + tail + b"\n")
    return b"".join(out)


@pytest.mark.gpu
def test_s5map_second_and_the_plain_lines(gpu, tmp_path):
    rng = np.random.default_rng(31)
    levels = rng.normal(90.0, 12.0, 800).astype(np.float32)
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("# expected levels\n\n" + "".join("%.9g\n" % v for v in levels))
    ref = quant_ref(levels)
    path = golden("example_multi_rg_v0.2.0.blow5")
    m = Blow5(path)
    n = len(m.records)
    dec = gpu.press.decode_to_device(m.records, m.rec_method, m.sig_method)
    ids = [g["read_id"] for g in gpu.press.decode_records(m.records, m.rec_method, m.sig_method)]
    counts = np.diff(gpu.events.events_dev(dec, DNA, "raw")[1].cpu().numpy())
    some = int(np.sort(counts)[n // 2])
    b_some = max(6, (some - 1).bit_length())
    for new, plain, skip, qmax, qmin, ws, b in ((["--second"], [], 0, 250, 50, False, 8),
                                                (["--second", "--block-shift", "6"], ["--start", "--events", "64", "--min-events", "20"], 0, 64, 20, True, 6),
                                                (["--second"], ["--start", "--events", str(some), "--min-events", str(some), "-K", "3"], 0, some, some, True, b_some)):
        want, want2, wst = _map2_want(gpu, dec, n, ref, skip, qmax, qmin, ws, b)
        p = subprocess.run([gpu.map.S5MAP] + new + plain + [str(ref_txt), path], capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stdout == _lines2(ids, want, want2, ws), new + plain
        # without the new options: byte for byte the lines of the tool as it was
        p = subprocess.run([gpu.map.S5MAP] + plain + [str(ref_txt), path], capture_output=True, timeout=120)
        assert p.returncode == 0 and p.stdout == map_lines(ids, want, ws), plain
    assert 0 < (want["qlen"] == 0).sum() < n
    got_ids, got = gpu.map.file_map(path, ref_txt, qmax=some, qmin=some, want_start=True)
    assert got_ids == ids and got.tolist() == want.tolist()
    for args in (["--block-shift", "6"], ["--second", "--block-shift", "5"], ["--second", "--block-shift", "31"], ["--fwd-only"], ["--second", "--block-shift"]):
        p = subprocess.run([gpu.map.S5MAP] + args + [str(ref_txt), path], capture_output=True, timeout=120)
        assert p.returncode == 2 and p.stdout == b"", args


@pytest.mark.gpu
def test_s5map_with_a_fasta_and_a_model(gpu, two_contigs, tmp_path):
    t = two_contigs
    path = golden("example_multi_rg_v0.2.0.blow5")
    m = Blow5(path)
    n = len(m.records)
    dec = gpu.press.decode_to_device(m.records, m.rec_method, m.sig_method)
    ids = [g["read_id"] for g in gpu.press.decode_records(m.records, m.rec_method, m.sig_method)]
    counts = np.diff(gpu.events.events_dev(dec, DNA, "raw")[1].cpu().numpy())
    some = int(np.sort(counts)[n // 2])
    for extra, kw, qmax, qmin in (([], dict(), 64, 20), (["--fwd-only"], dict(strands=1), 64, 20), (["--rna"], dict(rna=True), 64, 20), ([], dict(), some, some)):
        ref, segs, W = refseq_ref(t.contigs, t.model, t.k, **kw)
        b = max(6, (qmax - 1).bit_length())
        p = subprocess.run([gpu.map.S5MAP, "--fasta", str(t.fasta), "--model", str(t.model_path), "--events", str(qmax), "--min-events", str(qmin)] + extra + [path],
                           capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        want, want2, wst = _map2_want(gpu, dec, n, ref, 0, qmax, qmin, True, b, RNA if "--rna" in extra else DNA)     # (--rna: the tool's RNA event parameters too)
        lines = []
        for rid, r, s in zip(ids, want, want2):
            if r["qlen"] == 0:
                lines.append(rid + b"\t*" * 9 + b"\n")
                continue
            inside = [(c, st, o, l, rev) for c, st, o, l, rev in segs if o <= r["start"] and r["end"] < o + l]
            assert len(inside) == 1                                        # the wall property, on real reads
            c, st, o, l, rev = inside[0]
            a, e = int(r["start"]) - o, int(r["end"]) - o
            lo, hi = (l - 1 - e, l - 1 - a) if rev else (a, e)
            lines.append(b"%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%s\n" % (rid, r["qlen"], r["cost"], b"%.6g" % (float(r["cost"]) / float(r["qlen"])),
                                                                       t.contigs[c][0].encode(), st.encode(), lo, hi, s["mapq"],
                                                                       b"*" if s["end2"] < 0 else b"%d" % s["cost2"]))
        assert p.stdout == b"".join(lines), extra
    assert 0 < (want["qlen"] == 0).sum() < n
    # exit 2: an incomplete model, an unreadable one, an empty FASTA, no contig of k bases, --fasta without --model, a ref.txt beside --fasta
    write_model(tmp_path / "missing.model", t.model, t.k, skip=(3,))
    (tmp_path / "empty.fa").write_text("")
    (tmp_path / "short.fa").write_text(">x\nAC\n")
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("1.0\n2.0\n")
    for args in (["--fasta", str(t.fasta), "--model", str(tmp_path / "missing.model"), path], ["--fasta", str(t.fasta), "--model", str(tmp_path / "none.model"), path],
                 ["--fasta", str(tmp_path / "empty.fa"), "--model", str(t.model_path), path], ["--fasta", str(tmp_path / "short.fa"), "--model", str(t.model_path), path],
                 ["--fasta", str(t.fasta), path], ["--fasta", str(t.fasta), "--model", str(t.model_path), str(ref_txt), path]):
        p = subprocess.run([gpu.map.S5MAP] + args, capture_output=True, timeout=120)
        assert p.returncode == 2 and p.stdout == b"", args


@pytest.mark.gpu
def test_a_refseq_reference_goes_to_read_align_unchanged(gpu, two_contigs):
    t = two_contigs
    rs = gpu.map.RefSeq(fasta=t.fasta, model=t.model_path)
    m = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    rows, lo, hi, ev, st = gpu.align.read_align(m.records, rs.ref, m.rec_method, m.sig_method, qmax=64, qmin=10)
    rows2, sec, st2 = gpu.map.read_map2(m.records, rs, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True)
    assert rows.tolist() == rows2.tolist() and not st.any() and (rows["qlen"] == 64).all()
    spans = rs.spans(rows)
    for i, r in enumerate(rows):
        inside = [(c, name, s, o, l) for c, name, s, o, l in rs.segments if o <= lo[i, :64].min() and hi[i, :64].max() < o + l]
        assert len(inside) == 1 and spans[i] is not None and spans[i][0] == inside[0][0] and spans[i][1] == inside[0][2], i
        assert lo[i, 0] == r["start"] and hi[i, 63] == r["end"]
    with pytest.raises(ValueError, match="clip"):
        gpu.map.read_map2(m.records, rs, m.rec_method, m.sig_method, qmax=64, qmin=20, clip=100)


@pytest.mark.gpu
def test_refused_arguments_write_nothing(gpu):
    torch, L, lib = gpu.torch, gpu.L, gpu.lib
    vp = C.c_void_p
    n = 5
    d_q = torch.full((n, 64), 77, dtype=torch.int16, device="cuda")
    d_ql = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    d_out = torch.full((n * 4,), GUARD, dtype=torch.int32, device="cuda")
    d_out2 = torch.full((n * 4 + 4,), GUARD, dtype=torch.int32, device="cuda")
    d_ref = torch.zeros(100, dtype=torch.int16, device="cuda")

    def sdtw2(pitch=64, R=100, ref=True, q=True, bshift=6, out_off=0, out2=True, out2_off=0):
        return L.s5gpu_sdtw2_dev(n, d_q.data_ptr() if q else None, pitch, d_ql.data_ptr(), d_ref.data_ptr() if ref else None, R, 1, bshift,
                                 d_out.data_ptr() + out_off, d_out2.data_ptr() + out2_off if out2 else None, None)
    assert sdtw2(pitch=0) == -1 and sdtw2(pitch=1025) == -1 and sdtw2(R=0) == -1 and sdtw2(R=1 << 31) == -1 and sdtw2(ref=False) == -1 and sdtw2(q=False) == -1
    assert sdtw2(out_off=4) == -1 and sdtw2(out2=False) == -1 and sdtw2(out2_off=4) == -1 and sdtw2(out2_off=8) == -1
    for b in (0, 5, 31, 32, 0xFFFFFFFF):
        assert sdtw2(bshift=b) == -1, b
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (vp * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    h_ref = np.zeros(100, dtype=np.int16)
    h_rows, h_sec = np.full(16, 0xA5, dtype=np.uint8), np.full(16, 0xA5, dtype=np.uint8)
    h_st = np.full(1, -7, dtype=np.int32)

    def batch(pr=(0, 64, 10, 32.0, 127, 0), bshift=6, R=100, sec=True, rows=True):
        e, p = lib.EventParams(*DNA), lib.MapParams(*pr)
        return L.s5gpu_map2_batch(1, rec_p, rl, 1, 1, C.byref(e), C.byref(p), h_ref.ctypes.data_as(vp), R, bshift, h_rows.ctypes.data_as(vp) if rows else None,
                                  h_sec.ctypes.data_as(vp) if sec else None, h_st.ctypes.data_as(vp))
    assert batch(bshift=5) == -1 and batch(bshift=31) == -1 and batch(sec=False) == -1 and batch(rows=False) == -1 and batch(R=0) == -1
    assert batch(pr=(0, 1025, 1, 32.0, 127, 0)) == -1 and batch(pr=(0, 64, 10, 32.0, 0, 0)) == -1
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == GUARD).all() and (d_out2.cpu().numpy() == GUARD).all()                    # nothing was launched
    assert (h_rows == 0xA5).all() and (h_sec == 0xA5).all() and (h_st == -7).all()
    assert sdtw2(bshift=30) == 0 and sdtw2(out2_off=16) == 0
    torch.cuda.synchronize()
    o2 = d_out2.cpu().numpy()
    assert (o2[4:].view(MAP_SECOND)["end2"] == -1).all() and (d_out.cpu().numpy().view(MAP_ROW)["qlen"] == 7).all()
