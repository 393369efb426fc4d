"""model (docs/codecs.md §4.26): the fold of a table of pileup and of a level histogram onto classes (k_pile_fold, k_pile_hist_fold), the
classes and the quantiser of a reference made from sequences, the estimate of a level table, the folded closes of the handles and the two
tools.  Every output is held byte for byte to the restatements of fold_ref.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fold_ref as fr
from chain_common import ROOT, gpu, host_build, levels_signal, record, synth_file  # noqa: F401  (gpu: the fixture)
from contrast_ref import contrast_lines, contrast_ref, hist_bytes_of
from dtw_ref import quant_ref
from fold_ref import NONE, REFUSED, fold_cases, fold_ref, hist_fold_ref, table_bytes_of
from pileup_ref import table_bytes

CALLS = ["s5gpu_quant_stats_host", "s5gpu_refseq_classes", "s5gpu_refseq_quant", "s5gpu_pileup_fold_dev", "s5gpu_pile_hist_fold_dev", "s5gpu_pileup_close_folded",
         "s5gpu_contrast_close_folded", "s5gpu_kmer_model_solve"]
ERR_ARG = -1
DEFAULT_FOLD_LDS, DEFAULT_FOLD_GRID = 1, 512       # the library's defaults (docs/codecs.md §4.26, Measured)


def _explain(got, want):
    if len(got) != len(want):
        return "%d bytes, %d wanted" % (len(got), len(want))
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = int(np.flatnonzero(a != b)[0])
    return "first difference at byte %d (head 64): got %s, wanted %s" % (at, a[at:at + 8].tolist(), b[at:at + 8].tolist())


# ---------------------------------------------------------------------------------------------------------------- cpu

def test_library_exports_the_calls_and_the_tools_are_built(tmp_path):
    from slow5tools_amd import _lib, build, contrast, model

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported] and not [s for s in CALLS if s not in _lib.EXPORTS]
    src = tmp_path / "decl.c"
    src.write_text('#include "slow5gpu.h"\n#include <stdio.h>\nint main(void){\n'
                   'int (*a)(const void *, uint32_t, const uint32_t *, uint32_t, void *, void *) = s5gpu_pileup_fold_dev;\n'
                   'int (*b)(const void *, uint32_t, const uint32_t *, uint32_t, void *, void *) = s5gpu_pile_hist_fold_dev;\n'
                   'int (*c)(void *, const uint32_t *, uint32_t, void *) = s5gpu_pileup_close_folded;\n'
                   'int (*d)(void *, const uint32_t *, uint32_t, void *, void *, s5gpu_pile_contrast_t *) = s5gpu_contrast_close_folded;\n'
                   'int (*e)(const void *, uint32_t, double, double, double, uint32_t, const float *, s5gpu_kmer_row_t *) = s5gpu_kmer_model_solve;\n'
                   'int (*f)(const void *, uint32_t *, uint32_t *) = s5gpu_refseq_classes;\n'
                   'int (*g)(const void *, double *, double *, double *) = s5gpu_refseq_quant;\n'
                   'printf("%d %zu %u %u\\n", a && b && c && d && e && f && g, sizeof(s5gpu_kmer_row_t), S5GPU_FOLD_NONE, S5GPU_FOLD_REFUSED);return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == ["1", "40", str(NONE), "1"]
    # the tools: without arguments their usage (exit 2); bad options the same
    fa, md = str(tmp_path / "none.fa"), str(tmp_path / "none.model")
    p = subprocess.run([model.S5MODEL], capture_output=True)
    assert p.returncode == 2 and b"usage: s5model" in p.stderr and b"--min-cells" in p.stderr and p.stdout == b""
    good = ["--fasta", fa, "--model", md, "-o", str(tmp_path / "out.model"), str(tmp_path / "a.blow5")]
    for args in (["--iters", "0"], ["--iters", "17"], ["--min-cells", "0"], ["--tile", "100"], ["--band", "100"], ["--refine-iters", "5"], ["--bogus"]):
        p = subprocess.run([model.S5MODEL] + args + good, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr, (args, p.stderr)
    for args in (good[2:], good[:2] + good[4:], good[:4] + good[6:], good[:6]):                    # no --fasta, no --model, no -o, no file
        p = subprocess.run([model.S5MODEL] + args, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr, (args, p.stderr)
    p = subprocess.run([model.S5MODEL] + good, capture_output=True)                                # an unreadable model: no usage line
    assert p.returncode == 2 and b"usage" not in p.stderr and b"cannot" in p.stderr, p.stderr
    ab = [str(tmp_path / "a.blow5"), str(tmp_path / "b.blow5")]
    for args in (["--by-kmer", str(tmp_path / "ref.txt")] + ab, ["--fwd-only", str(tmp_path / "ref.txt")] + ab, ["--fasta", fa] + ab, ["--model", md] + ab,
                 ["--fasta", fa, "--model", md, "--by-kmer", str(tmp_path / "ref.txt")] + ab, ["--fasta", fa, "--model", md, "--by-kmer"] + ab[:1]):
        p = subprocess.run([contrast.S5CONTRAST] + args, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr and b"--by-kmer" in p.stderr and p.stdout == b"", (args, p.stderr)
    p = subprocess.run([contrast.S5CONTRAST, "--fasta", fa, "--model", md, "--by-kmer"] + ab, capture_output=True)
    assert p.returncode == 2 and b"usage" not in p.stderr and b"cannot" in p.stderr, p.stderr


def test_the_restatement_on_a_hand_made_table():
    total, cols = fr.empty_table(5)
    cols[0] = (1, 2, 10, -6, 20, 7, -4, -2)
    cols[1] = (2, 3, 30, 9, 29, 5, 2, 4)
    cols[3] = (1, 1, 5, 100, 10000, 1, 100, 100)
    cols[4] = (1, 1, 7, -32768, 32768 * 32768, 2, -32768, -32768)
    total["reads_used"], total["cells"], total["cost"] = 3, 7, 15
    t, c = fold_ref((total, cols), [1, 1, 0, NONE, 2], 3)
    assert c[1].tolist() == (3, 5, 40, 3, 49, 12, -4, 4) and c[0].tolist() == (0, 0, 0, 0, 0, 0, 32767, -32768) and c[2].tolist() == cols[4].tolist()
    assert (t["reads_used"], t["cells"], t["cost"], t["R"], t["reserved"][0]) == (3, 6, 14, 3, 0)
    t2, c2 = fold_ref((total, cols), [1, 1, 0, NONE, 2], 3, (t, c))            # the same input again: the sums doubled, the minima as they were
    assert c2[1].tolist() == (6, 10, 80, 6, 98, 24, -4, 4) and (t2["reads_used"], t2["cells"], t2["cost"]) == (6, 12, 28)
    total["cells"] = 2 ** 32
    t3, c3 = fold_ref((total, cols), [1, 1, 0, NONE, 2], 3)
    assert t3["reserved"][0] == REFUSED and table_bytes_of((t3, c3))[64:] == table_bytes_of(fr.empty_table(3))[64:] and t3["reads_used"] == 0
    for name, (table, hist, cls, K) in fold_cases().items():                   # the cases keep the invariants the tests rely on
        (t, c), (h, n) = fold_ref(table, cls, K), hist_fold_ref(hist, cls, K)
        assert n.sum(axis=1).tolist() == c["n_events"].tolist() and h["cells"] == t["cells"], name
        if name.startswith("none"):
            assert table_bytes_of((t, c))[64:] == table_bytes_of(fr.empty_table(K))[64:] and t["reads_used"] == table[0]["reads_used"] and t["cells"] == 0
        if name.startswith("lonely"):
            assert c[0].tolist() == (0, 0, 0, 0, 0, 0, 32767, -32768)
        if name.startswith("extreme") and len(cls) >= 63:
            assert c["min_q"].min() == -32768 and c["max_q"].max() == 32767


FOLD_HOST = r'''
// The code of k_pile_fold and k_pile_hist_fold that lives in fold_dev.h (and col_merge and window_slot of pileup_dev.h), on the CPU, with plain
// adds in place of the atomics: every column through fold_col into the class table (exactly K columns, when lds says so) or into the output
// (exactly K columns), the class table flushed at the end; every bin through fold_bin.  Every array is allocated at exactly its size.
// in.bin: R, K, lds, 0, then the input table, the input histogram, cls, the output table and the output histogram as they stand before;
// out.bin: the two outputs.
#define S5_PILEUP_HOST
#include "fold_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace pilek;
struct HostOps {
    static void add64(uint64_t *p, uint64_t v) { *p += v; }
    static void add32(uint32_t *p, uint32_t v) { *p += v; }
    static void minmax32(s5gpu_pile_col_t *c, int32_t lo, int32_t hi) { if (lo < c->min_q) c->min_q = lo; if (hi > c->max_q) c->max_q = hi; }
};
static void *get(FILE *f, size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) abort();
    return p;
}
int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t h[4];
    if (!f || !o || fread(h, 4, 4, f) != 4) return 1;
    const uint32_t R = h[0], K = h[1], lds = h[2];
    const size_t tb_in = 64 + 48 * (size_t)R, hb_in = 64 + 256 * (size_t)R, tb_out = 64 + 48 * (size_t)K, hb_out = 64 + 256 * (size_t)K;
    uint8_t *tin = (uint8_t *)get(f, tb_in), *hin = (uint8_t *)get(f, hb_in);
    uint32_t *cls = (uint32_t *)get(f, 4 * (size_t)R);
    uint8_t *tout = (uint8_t *)get(f, tb_out), *hout = (uint8_t *)get(f, hb_out);
    // the table
    s5gpu_pile_total_t *Ti = (s5gpu_pile_total_t *)tin, *To = (s5gpu_pile_total_t *)tout;
    const s5gpu_pile_col_t *ci = (const s5gpu_pile_col_t *)(tin + 64);
    s5gpu_pile_col_t *co = (s5gpu_pile_col_t *)(tout + 64);
    const uint32_t wcols = lds ? K : 0u;
    s5gpu_pile_col_t *win = (s5gpu_pile_col_t *)malloc(wcols ? wcols * sizeof *win : 1);
    for (uint32_t b = 0; b < wcols; b++) { memset(&win[b], 0, sizeof win[b]); win[b].min_q = 32767; win[b].max_q = -32768; }
    Window W;
    W.lo = 0; W.cols = lds ? FOLD_LDS_K : 0u;
    if (fold_heads_ok(Ti->cells, Ti->R, R, To->R, K)) {
        uint64_t cells = 0, cost = 0;
        for (uint32_t j = 0; j < R; j++) fold_col<HostOps>(ci[j], cls[j], K, W, win, co, &cells, &cost);
        for (uint32_t b = 0; b < wcols; b++) col_merge<HostOps>(co + b, win + b);
        To->reads_used += Ti->reads_used; To->reads_skipped += Ti->reads_skipped; To->reads_bad += Ti->reads_bad;
        To->cells += cells; To->cost += cost;
    } else To->reserved[0] |= S5GPU_FOLD_REFUSED;
    // the histogram
    s5gpu_pile_hist_head_t *Hi = (s5gpu_pile_hist_head_t *)hin, *Ho = (s5gpu_pile_hist_head_t *)hout;
    const uint32_t *bi = (const uint32_t *)(hin + 64);
    if (fold_heads_ok(Hi->cells, Hi->R, R, Ho->R, K) && fold_hist_heads_ok((const uint32_t *)hin, (const uint32_t *)hout)) {
        uint64_t cells = 0;
        for (uint32_t j = 0; j < R; j++)
            for (uint32_t b = 0; b < HIST_BINS; b++) cells += fold_bin<HostOps>(bi[(size_t)j * HIST_BINS + b], cls[j], K, b, (uint32_t *)(hout + 64));
        Ho->cells += cells; Ho->reads_used += Hi->reads_used; Ho->reads_skipped += Hi->reads_skipped; Ho->reads_bad += Hi->reads_bad;
    } else Ho->reserved[0] |= S5GPU_FOLD_REFUSED;
    fwrite(tout, 1, tb_out, o);
    fwrite(hout, 1, hb_out, o);
    free(tin); free(hin); free(cls); free(tout); free(hout); free(win);
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def _run_host(exe, tmp_path, table, hist, cls, K, lds, out_table=None, out_hist=None):
    out_table = fr.empty_table(K) if out_table is None else out_table
    out_hist = fr.empty_hist(K, int(hist[0]["q0"]), int(hist[0]["shift"])) if out_hist is None else out_hist
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<4I", len(cls), K, lds, 0) + table_bytes_of(table) + hist_bytes_of(hist) + np.asarray(cls, dtype="<u4").tobytes())
        fh.write(table_bytes_of(out_table) + hist_bytes_of(out_hist))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = (tmp_path / "out.bin").read_bytes()
    return raw[:64 + 48 * K], raw[64 + 48 * K:]


def refusal_cases():
    """(table, hist, cls, K, out_table, out_hist): an input whose head says 2^32 cells; histogram heads that disagree in q0, in shift"""
    table, hist, cls, K = fold_cases()["mixed R=65 K=4"]
    big_t, big_h = (np.array([table[0]])[0], table[1]), (np.array([hist[0]])[0], hist[1])
    big_t[0]["cells"] = big_h[0]["cells"] = 2 ** 32
    return [(big_t, big_h, cls, K, None, None), (table, hist, cls, K, None, fr.empty_hist(K, -127, 2)), (table, hist, cls, K, None, fr.empty_hist(K, -128, 3))]


def run_fold_header_on_the_cpu(tmp_path, extra=()):
    exe = host_build(tmp_path, "fold_host", FOLD_HOST, ["-O1", "-std=c++17", "-Wall"], extra, api=True)
    for name, (table, hist, cls, K) in fold_cases().items():
        want_t, want_h = table_bytes_of(fold_ref(table, cls, K)), hist_bytes_of(hist_fold_ref(hist, cls, K))
        for lds in (0, 1) if K <= 1024 else (0,):
            got_t, got_h = _run_host(exe, tmp_path, table, hist, cls, K, lds)
            assert got_t == want_t, (name, lds, _explain(got_t, want_t))
            assert got_h == want_h, (name, lds, _explain(got_h, want_h))
    # folded twice into one output; the refusals
    table, hist, cls, K = fold_cases()["mixed R=257 K=4"]
    once_t, once_h = fold_ref(table, cls, K), hist_fold_ref(hist, cls, K)
    got_t, got_h = _run_host(exe, tmp_path, table, hist, cls, K, 1, once_t, once_h)
    assert got_t == table_bytes_of(fold_ref(table, cls, K, once_t)) and got_h == hist_bytes_of(hist_fold_ref(hist, cls, K, once_h))
    for table, hist, cls, K, ot, oh in refusal_cases():
        got_t, got_h = _run_host(exe, tmp_path, table, hist, cls, K, 1, ot, oh)
        assert got_t == table_bytes_of(fold_ref(table, cls, K, ot)) and got_h == hist_bytes_of(hist_fold_ref(hist, cls, K, oh))


def test_the_header_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """fold_col, fold_bin and the heads' rules of fold_dev.h with col_merge and window_slot of pileup_dev.h as g++ compiles them, on every case
    of the GPU tests, with the class table and without"""
    run_fold_header_on_the_cpu(tmp_path)


def test_the_header_code_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: every table is allocated at exactly its size"""
    run_fold_header_on_the_cpu(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _levels(k, seed=5):
    return (90.0 + np.random.default_rng(seed).normal(0.0, 12.0, 4 ** k)).astype(np.float32)


def _seq(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def test_refseq_classes_and_quant():
    """s5gpu_refseq_classes against the rank restated in Python: a forward segment, a reverse-complement segment, the RNA rule, a k-mer with N,
    wall columns, a contig shorter than k, k = 1 and k = 10; s5gpu_refseq_quant reproduces RefSeq.ref through s5gpu_quantise_host"""
    from slow5tools_amd import _lib
    from slow5tools_amd import map as smap

    rng = np.random.default_rng(77)
    for k in (1, 3, 10):
        lv = _levels(k)
        s1 = _seq(rng, 60)
        contigs = [("a", s1), ("short", "ACGTACGTA"[:k - 1]), ("n", s1[:20] + "N" + s1[20:45] + "acgu"), ("b", _seq(rng, 33))]
        for strands, rna in ((2, False), (1, False), (2, True)):
            rs = smap.RefSeq(contigs=contigs, levels=lv, strands=strands, rna=rna)
            cls, K = rs.classes()
            want, wantK = fr.classes_ref(contigs, k, strands, rna)
            assert K == wantK == 4 ** k and cls.dtype == np.uint32 and cls.tolist() == want.tolist(), (k, strands, rna)
            walls = np.ones(len(cls), dtype=bool)
            for _, _, _, off, Lk in rs.segments:
                walls[off:off + Lk] = False
            assert walls.sum() == rs.wall * (len(rs.segments) - 1) and (cls[walls] == NONE).all() and (rs.ref[walls] == -32768).all()
            assert (cls[~walls] == NONE).sum() == k * (1 if rna or strands == 1 else 2)                          # the k-mers that hold the N
            # the class is the rank whose level the column took: the reference again, from the classes and the table
            lev = fr.levels_ref(cls[~walls], lv)
            assert rs.ref[~walls].tolist() == quant_ref(lev).tolist()
            q = np.zeros(len(lev), dtype=np.int16)
            assert _lib.lib().s5gpu_quantise_host(lev.ctypes.data_as(C.c_void_p), len(lev), 32.0, 127, q.ctypes.data_as(C.c_void_p)) == 0
            assert q.tolist() == rs.ref[~walls].tolist()
            # mu, sd and scale invert it: the same formula, value by value
            mu, sd, scale = rs.quant
            assert (mu, sd) == fr.quant_stats_ref(lev) and scale == 32.0
            z = np.clip(np.rint(((lev.astype(np.float64) - mu) / sd) * scale), -127, 127).astype(np.int16)
            assert z.tolist() == rs.ref[~walls].tolist()
            rs.close()
    assert _lib.lib().s5gpu_refseq_classes(None, None, None) == ERR_ARG and _lib.lib().s5gpu_refseq_quant(None, None, None, None) == ERR_ARG


def _solve_lib(cols, mu, sd, scale, levels, min_cells):
    from slow5tools_amd import model

    total = fr.empty_table(len(cols))[0]
    return model.solve((total, cols), (mu, sd, scale), levels, min_cells)


def test_solve_and_the_model_file(tmp_path):
    """s5gpu_kmer_model_solve against solve_ref on hand-made folded tables: n just below and at min_cells, var clamped at 0, extreme q;
    write_model followed by s5gpu_kmer_model_load returns the float32 levels"""
    from slow5tools_amd import _lib, model

    k, K = 2, 16
    lv = _levels(k, 9)
    _, cols = fr.empty_table(K)
    cols[1] = (3, 29, 290, 29 * 17, 29 * 17 * 17 + 40, 9, 10, 25)               # n = min_cells - 1: kept
    cols[2] = (3, 30, 300, 30 * 17, 30 * 17 * 17 + 40, 9, 10, 25)               # n = min_cells
    cols[3] = (1, 30, 0, 30 * 5, 30 * 25, 0, 5, 5)                              # var exactly 0
    cols[4] = (1, 3, 7, 10, 33, 0, 3, 4)                                        # sumsq / n - mean^2 below 0 in floating point: clamped
    cols[5] = (1, 31, 1, -32768 * 31, 32768 * 32768 * 31, 0, -32768, -32768)    # extreme q
    cols[6] = (1, 40, 2 ** 40, 32767 * 40, 32767 * 32767 * 40, 0, 32767, 32767)
    cols[7] = (1, 2 ** 32 - 1, 2 ** 60, -(2 ** 40), 2 ** 63, 0, -127, 127)
    cols[8] = (1, 1, 3, -7, 49, 0, -7, -7)
    for min_cells in (30, 3, 1, 0):
        mu, sd, scale = 91.25, 11.5, 32.0
        got, want = _solve_lib(cols, mu, sd, scale, lv, min_cells), fr.solve_ref(cols, mu, sd, scale, lv, min_cells)
        assert got.tobytes() == want.tobytes(), (min_cells, got, want)
    got = _solve_lib(cols, 91.25, 11.5, 32.0, lv, 30)
    assert got["kept"].tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 1] + [1] * 7 and got["level"][1] == float(lv[1]) and got["stdv"][3] == 0.0 and got["level"][0] == float(lv[0])
    assert got["level"][2] == 91.25 + (11.5 / 32.0) * 17.0 and got["dwell"][2] == 10.0
    L, vp = _lib.lib(), C.c_void_p
    raw = np.frombuffer(table_bytes_of((fr.empty_table(K)[0], cols)), dtype=np.uint8).copy()
    rows = np.zeros(K, dtype=model.KMER_ROW)
    for bad in (dict(K=0), dict(sd=0.0), dict(sd=float("nan")), dict(scale=-1.0), dict(K=15), dict(acc=None), dict(lv=None), dict(rows=None)):
        a = dict(acc=raw.ctypes.data_as(vp), K=K, mu=0.0, sd=1.0, scale=32.0, lv=lv.ctypes.data_as(vp), rows=rows.ctypes.data_as(vp))
        a.update(bad)
        assert L.s5gpu_kmer_model_solve(a["acc"], a["K"], a["mu"], a["sd"], a["scale"], 30, a["lv"], a["rows"]) == ERR_ARG, bad
    # the file
    path = tmp_path / "t.model"
    model.write_model(path, k, got, occurrences=np.arange(K), reads_used=12, rounds=2)
    text = path.read_text().split("\n")
    assert text[0] == "# s5model k=2 reads_used=12 rounds=2" and text[1].split("\t") == ["kmer", "level_mean", "level_stdv", "cells", "occurrences", "dwell", "kept"]
    assert text[2].split("\t")[0] == "AA" and text[17].split("\t")[0] == "TT" and text[4].split("\t")[3:] == ["30", "2", "10", "0"]
    p, kk = C.POINTER(C.c_float)(), C.c_uint32()
    assert L.s5gpu_kmer_model_load(os.fsencode(path), C.byref(p), C.byref(kk)) == 0 and kk.value == k
    back = np.ctypeslib.as_array(p, (K,)).copy()
    L.s5gpu_kmer_model_free(p)
    assert back.tolist() == got["level"].astype(np.float32).tolist()
    k2, t = model.read_model(path)
    assert k2 == k and t["kmer"].tolist() == [model.kmer_of(r, k).encode() for r in range(K)] and t["cells"].tolist() == got["cells"].tolist()
    assert t["level_mean"].astype(np.float32).tolist() == back.tolist() and t["occurrences"].tolist() == list(range(K)) and t["kept"].tolist() == got["kept"].tolist()


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def test_the_planted_round():
    """One round on a planted table, wholly on the restatements (band_ref, pileup_long_ref, fold_ref, solve_ref): over the k-mers that
    reached min_cells the estimate lies closer to the truth than the table the reference was made from; the library's solve agrees with
    the restatement on the folded table.  Measured: all 64 k-mers reached min_cells; rms(A - truth) 3.5084, rms(estimate - truth) 1.8219
    (no refinement: each read carries the scale error of its own quantiser)."""
    p = fr.planted_round()
    rows, A, truth = p["rows"], p["A"], p["truth"]
    at = rows["kept"] == 0
    before, after = _rms(A[at].astype(np.float64) - truth[at]), _rms(rows["level"][at] - truth[at])
    print("planted round: %d of %d k-mers reached min_cells; rms(A - truth) %.4f, rms(estimate - truth) %.4f" % (at.sum(), len(at), before, after))
    got = _solve_lib(p["folded"][1], p["mu"], p["sd"], 32.0, A, 30)
    assert got.tobytes() == rows.tobytes()
    assert at.sum() >= 32 and after < before


def test_refused_arguments_are_refused_before_a_launch():
    """every S5GPU_ERR_ARG case of the two device calls returns before anything is launched: no device is needed, no pointer is followed"""
    from slow5tools_amd import _lib

    L, P = _lib.lib(), 0x10000

    def fold(call, i=P, R=100, cls=P + 0x1000, K=10, o=P + 0x2000):
        return call(i, R, cls, K, o, None)
    for call, most in ((L.s5gpu_pileup_fold_dev, 1 << 26), (L.s5gpu_pile_hist_fold_dev, 1 << 22)):
        for bad in (dict(i=None), dict(cls=None), dict(o=None), dict(i=P + 8), dict(o=P + 0x2008), dict(cls=P + 0x1002), dict(R=0), dict(K=0), dict(R=most + 1),
                    dict(K=most + 1), dict(o=P)):
            assert fold(call, **bad) == ERR_ARG, bad
            assert _lib.lib().s5gpu_last_error()
    assert L.s5gpu_pileup_close_folded(None, None, 4, None) == ERR_ARG and L.s5gpu_contrast_close_folded(None, None, 4, None, None, None) == ERR_ARG
    for key, bad in ((b"pile_fold_lds", (2, -1)), (b"pile_fold_grid", (0, 1025))):
        for v in bad:
            assert L.s5gpu_set_option(key, v) == ERR_ARG
    assert L.s5gpu_set_option(b"pile_fold_lds", DEFAULT_FOLD_LDS) == 0 and L.s5gpu_set_option(b"pile_fold_grid", DEFAULT_FOLD_GRID) == 0


# ---------------------------------------------------------------------------------------------------------------- gpu

class Guarded:
    """`raw` on the device between two guards of 64 bytes of 0x5A"""

    def __init__(self, env, raw):
        self.env, self.nb = env, len(raw)
        h = np.full(self.nb + 128, 0x5A, dtype=np.uint8)
        h[64:64 + self.nb] = np.frombuffer(raw, dtype=np.uint8)
        self.t = env.torch.from_numpy(h).to("cuda")
        self.ptr = self.t.data_ptr() + 64
        assert self.ptr % 16 == 0

    def bytes(self):
        self.env.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:64] == 0x5A).all() and (h[-64:] == 0x5A).all(), "a guard was written"
        return h[64:-64].tobytes()


def _options(env, lds=DEFAULT_FOLD_LDS, grid=DEFAULT_FOLD_GRID):
    for key, v in ((b"pile_fold_lds", lds), (b"pile_fold_grid", grid)):
        env.lib.check(env.L.s5gpu_set_option(key, v), key.decode())


def _fold_on_device(env, table, hist, cls, K, out_table=None, out_hist=None, times=1):
    """both folds through the C calls, `times` times into one output, every buffer between guards and the inputs checked afterwards"""
    tin, hin = Guarded(env, table_bytes_of(table)), Guarded(env, hist_bytes_of(hist))
    c = Guarded(env, np.asarray(cls, dtype="<u4").tobytes())
    tout = Guarded(env, table_bytes_of(fr.empty_table(K) if out_table is None else out_table))
    hout = Guarded(env, hist_bytes_of(fr.empty_hist(K, int(hist[0]["q0"]), int(hist[0]["shift"])) if out_hist is None else out_hist))
    for _ in range(times):
        assert env.L.s5gpu_pileup_fold_dev(tin.ptr, len(cls), c.ptr, K, tout.ptr, None) == 0, env.L.s5gpu_last_error()
        assert env.L.s5gpu_pile_hist_fold_dev(hin.ptr, len(cls), c.ptr, K, hout.ptr, None) == 0, env.L.s5gpu_last_error()
    got = tout.bytes(), hout.bytes()
    assert tin.bytes() == table_bytes_of(table) and hin.bytes() == hist_bytes_of(hist) and c.bytes() == np.asarray(cls, dtype="<u4").tobytes(), "an input was written"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("R", fr.RS)
def test_the_case_list_is_exact(gpu, R):
    """every K, class map and content at this R, under both values of pile_fold_lds (and a grid of one workgroup): byte for byte fold_ref"""
    try:
        for name, (table, hist, cls, K) in fold_cases().items():
            if len(cls) != R:
                continue
            want = table_bytes_of(fold_ref(table, cls, K)), hist_bytes_of(hist_fold_ref(hist, cls, K))
            outs = []
            for lds, grid in ((0, DEFAULT_FOLD_GRID), (1, DEFAULT_FOLD_GRID), (1, 1)):
                _options(gpu, lds, grid)
                got = _fold_on_device(gpu, table, hist, cls, K)
                assert got[0] == want[0], (name, lds, grid, _explain(got[0], want[0]))
                assert got[1] == want[1], (name, lds, grid, _explain(got[1], want[1]))
                outs.append(got)
            assert outs[0] == outs[1] == outs[2]
    finally:
        _options(gpu)


@pytest.mark.gpu
def test_twice_refused_and_the_argument_errors(gpu):
    try:
        for lds in (0, 1):
            _options(gpu, lds)
            # the same input folded twice: doubled sums, unchanged minima
            table, hist, cls, K = fold_cases()["mixed R=1025 K=1024"]
            once_t, once_h = fold_ref(table, cls, K), hist_fold_ref(hist, cls, K)
            twice_t, twice_h = fold_ref(table, cls, K, once_t), hist_fold_ref(hist, cls, K, once_h)
            got = _fold_on_device(gpu, table, hist, cls, K, times=2)
            assert got == (table_bytes_of(twice_t), hist_bytes_of(twice_h))
            assert twice_t[1]["n_events"].tolist() == (2 * once_t[1]["n_events"]).tolist() and twice_t[1]["min_q"].tolist() == once_t[1]["min_q"].tolist()
            # 2^32 cells in the head, histogram heads that disagree: nothing added, S5GPU_FOLD_REFUSED set
            for k, (table, hist, cls, K, ot, oh) in enumerate(refusal_cases()):
                got = _fold_on_device(gpu, table, hist, cls, K, ot, oh)
                want_t, want_h = fold_ref(table, cls, K, ot), hist_fold_ref(hist, cls, K, oh)
                assert got == (table_bytes_of(want_t), hist_bytes_of(want_h)), k
                assert want_h[0]["reserved"][0] == REFUSED and want_h[1].sum() == 0 and (want_t[0]["reserved"][0] == REFUSED) == (k == 0)
        # every S5GPU_ERR_ARG case returns before a launch: the outputs stay as they were
        table, hist, cls, K = fold_cases()["mixed R=65 K=4"]
        tin, c, tout = Guarded(gpu, table_bytes_of(table)), Guarded(gpu, np.asarray(cls, dtype="<u4").tobytes()), Guarded(gpu, table_bytes_of(fr.empty_table(K)))
        hin, hout = Guarded(gpu, hist_bytes_of(hist)), Guarded(gpu, hist_bytes_of(fr.empty_hist(K)))
        for call, i, o, most in ((gpu.L.s5gpu_pileup_fold_dev, tin, tout, 1 << 26), (gpu.L.s5gpu_pile_hist_fold_dev, hin, hout, 1 << 22)):
            for a in ((None, 65, c.ptr, K, o.ptr), (i.ptr, 65, None, K, o.ptr), (i.ptr, 65, c.ptr, K, None), (i.ptr + 8, 65, c.ptr, K, o.ptr), (i.ptr, 65, c.ptr + 2, K, o.ptr),
                      (i.ptr, 65, c.ptr, K, o.ptr + 4), (i.ptr, 0, c.ptr, K, o.ptr), (i.ptr, 65, c.ptr, 0, o.ptr), (i.ptr, most + 1, c.ptr, K, o.ptr),
                      (i.ptr, 65, c.ptr, most + 1, o.ptr), (i.ptr, 65, c.ptr, K, i.ptr)):
                assert call(*a, None) == ERR_ARG, a
        assert tout.bytes() == table_bytes_of(fr.empty_table(K)) and hout.bytes() == hist_bytes_of(fr.empty_hist(K)) and tin.bytes() == table_bytes_of(table)
    finally:
        _options(gpu)


@pytest.mark.gpu
def test_a_folded_pair_through_the_unchanged_comparison(gpu):
    """model.fold_dev and hist_fold_dev on two sides; the bins of every folded column add up to its n_events; contrast.contrast_dev on the
    folded pair equals contrast_ref on the folded restatements"""
    from slow5tools_amd import model

    torch, ct, pl = gpu.torch, gpu.contrast, gpu.pileup
    ta, ha, cls, K = fold_cases()["mixed R=257 K=4"]
    tb, hb, _, _ = fold_cases()["extreme R=257 K=4"]
    dev = lambda raw: torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to("cuda")   # noqa: E731
    accs = [model.fold_dev(dev(table_bytes_of(t)), cls, K) for t in (ta, tb)]
    hists = [model.hist_fold_dev(dev(hist_bytes_of(h)), cls, K) for h in (ha, hb)]
    want_t, want_h = [fold_ref(t, cls, K) for t in (ta, tb)], [hist_fold_ref(h, cls, K) for h in (ha, hb)]
    for s in (0, 1):
        total, cols = pl.to_host(accs[s])
        head, counts = ct.hist_to_host(hists[s])
        assert table_bytes((total, cols)) == table_bytes_of(want_t[s]) and hist_bytes_of((head, counts)) == hist_bytes_of(want_h[s])
        assert counts.sum(axis=1).tolist() == cols["n_events"].tolist() and head["cells"] == total["cells"] and not model.refused(total) and not model.refused(head)
    rows = ct.rows_to_host(ct.contrast_dev(hists[0], hists[1], accs[0], accs[1]))
    want = contrast_ref(want_h[0][1], want_h[1][1], want_t[0][1], want_t[1][1])
    assert rows.tobytes() == want.tobytes() and (rows["n_a"] > 0).all() and not (rows["flags"] & ~np.uint16(7)).any()
    # a device tensor of classes, and an output given: the fold adds
    c = torch.from_numpy(np.asarray(cls, dtype=np.uint32).view(np.int32)).to("cuda")
    again = model.fold_dev(dev(table_bytes_of(ta)), c, K, out=accs[0])
    assert again is accs[0] and table_bytes(pl.to_host(again)) == table_bytes_of(fold_ref(ta, cls, K, want_t[0]))
    with pytest.raises(ValueError):
        model.fold_dev(dev(table_bytes_of(ta)), cls[:-1], K)


KW = dict(skip=2, qmax=100, qmin=20, tile_rows=64, band=128)
TOOL_ARGS = ["--skip", "2", "--events", "100", "--min-events", "20", "--tile", "64", "--band", "128"]


@pytest.fixture(scope="module")
def chain(gpu, tmp_path_factory):
    """a small synthetic file of 16 reads (one too short for a query), a FASTA file of one contig and a table of k = 3"""
    from slow5tools_amd import model

    d = tmp_path_factory.mktemp("fold")
    rng = np.random.default_rng(4026)
    env = type("Chain", (), {})()
    env.k, env.levels = 3, _levels(3, 21)
    env.fasta, env.model = str(d / "ref.fa"), str(d / "in.model")
    seq = _seq(rng, 900)
    with open(env.fasta, "w") as fh:
        fh.write(">contig one\n" + "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + "\n")
    with open(env.model, "w") as fh:
        fh.write("".join("%s\t%.9g\n" % (model.kmer_of(r, 3), env.levels[r]) for r in range(64)))
    env.recs = [record(i, levels_signal(100 if i == 5 else int(rng.integers(5000, 8000)), rng)) for i in range(16)]
    env.rs = gpu.map.RefSeq(fasta=env.fasta, model=env.model)
    env.cls, env.K = env.rs.classes()
    env.dir = d
    assert env.K == 64 and len(env.rs.ref) == 2 * 898 + env.rs.wall
    return env


@pytest.mark.gpu
def test_the_handles_close_folded(gpu, chain):
    """Pileup, PileupWhole and Contrast: close_folded equals fold_ref of what close returns, on the same file: two handles each"""
    pl, ct = gpu.pileup, gpu.contrast
    ref, cls, K = chain.rs.ref, chain.cls, chain.K
    for make in (lambda: pl.Pileup(ref, skip=2, qmax=100, qmin=20), lambda: pl.PileupWhole(ref, **KW)):
        with make() as h:
            h.add(chain.recs)
            table = h.close()
        with make() as h:
            h.add(chain.recs[:7])
            h.add(chain.recs[7:])
            folded = h.close_folded(cls, K)
            assert h._h is None
        assert table[0]["reads_used"] == 15 and table[0]["reads_skipped"] == 1 and table[0]["cells"] > 1000
        assert table_bytes(folded) == table_bytes_of(fold_ref(table, cls, K)) and 0 < folded[0]["cells"] <= table[0]["cells"]
        with make() as h:                                                  # a bad class array ends the handle too
            with pytest.raises(ValueError):
                h.close_folded(cls[:-1], K)
            assert h._h is None
    sides = (chain.recs[:8], chain.recs[8:])
    with ct.Contrast(ref, **KW) as h:
        for s in (0, 1):
            h.add(s, sides[s])
        rows, a, b = h.close()
    with ct.Contrast(ref, **KW) as h:
        for s in (1, 0):
            h.add(s, sides[s])
        frows, fa, fb = h.close_folded(cls, K)
    assert table_bytes(fa) == table_bytes_of(fold_ref(a, cls, K)) and table_bytes(fb) == table_bytes_of(fold_ref(b, cls, K))
    # the histograms never come to the host: the rows of the folded tables' histograms, restated from PileupWhole's chain
    dec =[gpu.press.decode_to_device(x) for x in sides]
    _, accs, hs = ct.contrast_whole_dev(dec[0], dec[1], ref, **KW)
    hists = [hist_fold_ref(ct.hist_to_host(x), cls, K) for x in hs]
    want = contrast_ref(hists[0][1], hists[1][1], fa[1], fb[1])
    assert frows.tobytes() == want.tobytes() and len(frows) == K and (frows["n_a"] == fa[1]["n_events"]).all() and not (frows["flags"] & 48).any()
    assert [table_bytes(pl.to_host(x)) for x in accs] == [table_bytes(a), table_bytes(b)]


def _python_round(gpu, chain, cur, out, rounds_done, min_cells):
    """a round as the tool makes it, through PileupWhole, fold_dev and solve"""
    from slow5tools_amd import model

    rs = gpu.map.RefSeq(fasta=chain.fasta, model=cur)
    cls, K = rs.classes()
    _, t = model.read_model(cur)
    with gpu.pileup.PileupWhole(rs.ref, **KW) as h:
        h.add(chain.recs)
        table = h.close()
    acc = gpu.torch.from_numpy(np.frombuffer(table_bytes(table), dtype=np.uint8).copy()).to("cuda")
    folded = gpu.pileup.to_host(model.fold_dev(acc, cls, K))
    rows = model.solve(folded, rs, t["level_mean"].astype(np.float32), min_cells)
    model.write_model(out, rs.k, rows, model.occurrences(cls, K), folded[0]["reads_used"], rounds_done)
    rs.close()
    return rows


@pytest.mark.gpu
def test_the_tools(gpu, chain):
    """s5model at --iters 1 and 2 writes the table the Python chain gives, line for line; s5contrast --by-kmer prints the lines made from
    close_folded's rows"""
    from slow5tools_amd import model

    d = chain.dir
    synth_file(d / "all.blow5", chain.recs)
    cur = chain.model
    for n in (1, 2):
        py, out = str(d / ("py%d.model" % n)), str(d / ("tool%d.model" % n))
        rows = _python_round(gpu, chain, cur, py, n, 5)
        p = subprocess.run([model.S5MODEL, "-K", "5", "--iters", str(n), "--min-cells", "5"] + TOOL_ARGS + ["--fasta", chain.fasta, "--model", chain.model, "-o", out,
                            str(d / "all.blow5")], capture_output=True, timeout=120)
        assert p.returncode == 0 and b"round %d: reads used 15, skipped 1, bad 0" % n in p.stderr, p.stderr
        assert open(out).read() == open(py).read()
        assert (rows["kept"] == 0).sum() > 32 and (rows["level"] != chain.levels).any()
        cur = py
    k, t = model.file_model(d / "all.blow5", chain.fasta, chain.model, d / "fm.model", batch=16, iters=2, min_cells=5, tile_rows=64, band=128, skip=2, qmax=100, qmin=20)
    assert k == 3 and open(d / "fm.model").read() == open(d / "tool2.model").read() and t["occurrences"].tolist() == model.occurrences(chain.cls, chain.K).tolist()
    # s5contrast --by-kmer
    ct = gpu.contrast
    sides = (chain.recs[:8], chain.recs[8:])
    for s, name in enumerate(("a.blow5", "b.blow5")):
        synth_file(d / name, sides[s])
    with ct.Contrast(chain.rs.ref, **KW) as h:
        for s in (0, 1):
            h.add(s, sides[s])
        rows, a, b = h.close_folded(chain.cls, chain.K)
    kq = np.zeros(chain.K, dtype=np.int16)
    kq[chain.cls[chain.cls < chain.K]] = chain.rs.ref[chain.cls < chain.K]
    at = np.flatnonzero((rows["depth_a"] >= 1) & (rows["depth_b"] >= 1))
    want = [model.kmer_of(j, 3).encode() + ln[ln.index(b"\t"):] for j, ln in zip(at, contrast_lines(kq, rows, a[1], b[1]))]
    p = subprocess.run([ct.S5CONTRAST, "-K", "3"] + TOOL_ARGS + ["--fasta", chain.fasta, "--model", chain.model, "--by-kmer", str(d / "a.blow5"), str(d / "b.blow5")],
                       capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"".join(want) and len(want) > 32, p.stderr
    # ... and without --by-kmer the per-column lines of the same reference
    with ct.Contrast(chain.rs.ref, **KW) as h:
        for s in (0, 1):
            h.add(s, sides[s])
        rows, a, b = h.close()
    p = subprocess.run([ct.S5CONTRAST, "-K", "3"] + TOOL_ARGS + ["--fasta", chain.fasta, "--model", chain.model, str(d / "a.blow5"), str(d / "b.blow5")],
                       capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"".join(contrast_lines(chain.rs.ref, rows, a[1], b[1])), p.stderr
