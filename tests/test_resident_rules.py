"""The rules of the resident-decode front, without a GPU: csrc/resident_rules.h compiled on its own with a small main, against the rules as the
host files carried them before the header existed (restated here in Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slow5tools_amd", "csrc")
OK, ERR_ARG, ERR_HIP, ERR_DATA = 0, -1, -2, -5
U64 = 2 ** 64

# (name, chunk_bytes, [(pos, len)]): an empty batch; a record that ends exactly at chunk_bytes, and one a byte past it; pos > chunk_bytes;
# pos + len wrapping 64 bits (a pos only a chunk of 2^64 - 1 bytes allows; the wrapped end is below the true one); a b0 that is not 16-aligned
SPANS = [
    ("empty", 1000, []),
    ("ends_at_the_end", 1000, [(16, 100), (900, 100)]),
    ("one_byte_past", 1000, [(16, 100), (900, 101)]),
    ("pos_past", 1000, [(8, 8), (1001, 0)]),
    ("pos_at_the_end", 1000, [(1000, 0)]),
    ("wraps", 2 ** 64 - 1, [(40, 2), (2 ** 64 - 8, 100)]),
    ("wraps_inside", 2 ** 64 - 1, [(2 ** 64 - 8, 7), (2 ** 64 - 100, 50)]),
    ("unaligned", 4096, [(523, 77), (41, 9), (700, 1)]),
    ("aligned", 4096, [(48, 16), (32, 1)]),
]

# one attempt's fields over a batch: (status, payload_len, n_samples); the table is run for attempts 0, 1 and 2 from the same slots
GROW_SLOTS = [(5000, 5000), (5000, 9000), (0x0FFFFFFF, 0x0FFFFFFF), (0x10000000, 0x10000000), (0xFFFFFF00, 0xFFFFFF00), (64, 64), (64, 64), (64, 64), (64, 64)]
GROW_FIELDS = [(5, 70000, 0), (5, 0, 0), (5, 0, 0), (5, 0, 0), (5, 0xFFFFFFFF, 0), (6, 40, 3000), (0, 40, 30), (3, 0, 0), (5, 0, 0)]
GUESSES = [0, 1, 4096, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFF01, 2 ** 40]

# the dropping loop: per round, the status of every record of the batch as the fake decode reports it (None: the round must not happen)
DROPS = [
    ("none", 0, []),
    ("all_good", 3, [[0, 0, 0]]),
    ("corrupt_only", 3, [[0, 2, 0]]),
    ("unfinished_only", 3, [[0, 5, 6]]),
    ("corrupt_and_unfinished", 5, [[0, 3, 5, 0, 6], [0, None, 0, 0, 0]]),
    ("second_round_finds_more", 5, [[0, 3, 5, 0, 6], [0, None, 4, 0, 6], [0, None, None, 0, 0]]),
    ("four_rounds", 6, [[2, 5, 0, 0, 0, 0], [None, 5, 3, 0, 0, 0], [None, 5, None, 4, 0, 0], [None, 5, None, None, 1, 0]]),
    ("hard_error", 3, [[0, 2, 5], "hip"]),
]

PROBE = r"""
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "resident_rules.h"
static char g_err[256];
extern "C" void s5gpu_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
struct Span { const char *name; uint64_t bytes; uint32_t n; uint64_t pos[4]; uint32_t len[4]; };
struct Drop { const char *name; uint32_t n; int rounds; int st[4][8]; };     // st < 0: -1 the record is not in the round, -2 the decode fails hard
int main() {
    for (int r = 0; r < 3; r++)
        for (int s = 0; s < 3; s++) printf("methods %%d %%d %%d %%d\n", r, s, (int)s5rules::methods_ok(r, s), (int)s5rules::decodes_without_payload(r, s));
    printf("methods -1 0 %%d 0\nmethods 3 1 %%d 0\nmethods 1 3 %%d 0\nmethods 0 -1 %%d 0\n", (int)s5rules::methods_ok(-1, 0), (int)s5rules::methods_ok(3, 1),
           (int)s5rules::methods_ok(1, 3), (int)s5rules::methods_ok(0, -1));
    const Span spans[] = {%(spans)s};
    for (const Span &S : spans) {
        uint64_t b0 = 77, e1 = 77;
        g_err[0] = 0;
        const int rc = s5rules::chunk_span("who", "thing", S.n, (size_t)S.bytes, S.pos, S.len, &b0, &e1);
        printf("span %%s %%d %%llu %%llu %%d|%%s\n", S.name, rc, (unsigned long long)b0, (unsigned long long)e1, s5rules::chunk_span("who", "thing", S.n, (size_t)S.bytes,
               S.pos, S.len, nullptr, nullptr), g_err);
    }
    const void *recs[3] = {"a", nullptr, nullptr};
    const size_t lens[3] = {1, 0, 4};
    g_err[0] = 0;
    printf("records %%d %%d|%%s\n", s5rules::host_records_ok("who", 2, recs, lens), s5rules::host_records_ok("who", 3, recs, lens), g_err);
    const uint64_t guesses[] = {%(guesses)s};
    for (uint64_t g : guesses) printf("first %%llu %%u\n", (unsigned long long)g, s5rules::first_cap(g));
    const uint32_t slots[][2] = {%(slots)s};
    const s5gpu_rec_fields_t fields[] = {%(fields)s};
    const uint32_t nf = sizeof fields / sizeof fields[0];
    for (int attempt = 0; attempt < 3; attempt++) {
        uint32_t pcap[nf], scap[nf];
        int32_t status[nf];
        for (uint32_t i = 0; i < nf; i++) { pcap[i] = slots[i][0]; scap[i] = slots[i][1]; status[i] = -9; }
        bool bad = false;
        const bool retry = s5rules::grow_batch(nf, fields, attempt, pcap, scap, status, &bad);
        printf("grow %%d %%d %%d", attempt, (int)retry, (int)bad);
        for (uint32_t i = 0; i < nf; i++) printf(" %%u,%%u,%%d", pcap[i], scap[i], status[i]);
        printf("\n");
    }
    { bool bad = false; uint32_t p = 64, s = 64; s5gpu_rec_fields_t f; memset(&f, 0, sizeof f); f.status = 2;   // no status array: not written
      const bool retry = s5rules::grow_batch(1, &f, 0, &p, &s, nullptr, &bad);
      printf("grow_null %%d %%d\n", (int)retry, (int)bad); }
    const Drop drops[] = {%(drops)s};
    for (const Drop &D : drops) {
        std::vector<s5gpu_rec_fields_t> ff;
        std::vector<uint32_t> cur;
        int32_t status[8];
        for (int i = 0; i < 8; i++) status[i] = -9;
        bool corrupt = false;
        int round = 0;
        printf("drop %%s", D.name);
        const int rc = s5rules::decode_dropping_corrupt(D.n, [&](uint32_t m, const uint32_t *idx) {
            printf(" [");
            for (uint32_t k = 0; k < m; k++) printf("%%s%%u", k ? "," : "", idx[k]);
            printf("]");
            if (round >= D.rounds) { printf(" TOO_MANY"); return -2; }
            const int *st = D.st[round++];
            if (st[0] == -2) return -2;
            ff.resize(m);
            bool bad = false;
            for (uint32_t k = 0; k < m; k++) { memset(&ff[k], 0, sizeof ff[k]); ff[k].status = st[idx[k]]; bad |= st[idx[k]] != 0; }
            return bad ? -5 : 0;
        }, ff, cur, status, &corrupt);
        printf(" rc=%%d corrupt=%%d cur=", rc, (int)corrupt);
        for (size_t k = 0; k < cur.size(); k++) printf("%%s%%u", k ? "," : "", cur[k]);
        printf(" ff=%%zu status=", ff.size());
        for (uint32_t i = 0; i < D.n; i++) printf("%%s%%d", i ? "," : "", status[i]);
        printf("\n");
    }
    return 0;
}
"""


def _methods_ok(rec, sig):
    """the whitelist every *_api.hip file spelled out"""
    return rec in (0, 1, 2) and sig in (0, 1, 2)


def _no_payload(rec, sig):
    """signal_api.hip, fstats_api.hip: zlib / zstd + svb-zd and zlib + ex-zd"""
    return (sig == 1 and rec in (1, 2)) or (sig == 2 and rec == 1)


def _span(chunk_bytes, items):
    """the loop of the chunk calls: (rc, b0, e1, first bad item); b0 / e1 untouched (77) when an item lies outside"""
    b0, e1 = (U64 - 1 if items else 0), 0
    for i, (pos, ln) in enumerate(items):
        if pos > chunk_bytes or ln > chunk_bytes - pos:
            return ERR_ARG, 77, 77, i
        b0, e1 = min(b0, pos), max(e1, pos + ln)
    return OK, b0 & ~15, e1, None


def _grow(attempt):
    """decode_resident_impl / decode_np_framed after one attempt: (retry, bad, [(pcap, scap, status)])"""
    retry = bad = False
    out = []
    for (pcap, scap), (st, plen, ns) in zip(GROW_SLOTS, GROW_FIELDS):
        seen = -9
        if st == 5 and attempt < 2:
            pcap = plen if plen > pcap else (8 * pcap + 65536 if pcap < 0x10000000 else 0xFFFFFF00)
            scap = max(scap, pcap)
            retry = True
        elif st == 6 and attempt < 2:
            scap = ns
            retry = True
        elif st != 0:
            bad, seen = True, st
        out.append((pcap, scap, seen))
    return retry, bad, out


def _drop(n, rounds):
    """decode_dropping_corrupt as host_ctx.h had it: the line the probe prints"""
    cur, status, corrupt, ff_len, line, rc = list(range(n)), [-9] * n, False, 0, "", OK
    for r in range(4):
        if cur:
            line += " [" + ",".join(map(str, cur)) + "]"
            if rounds[r] == "hip":
                rc = ERR_HIP
                break
            st = [rounds[r][i] for i in cur]
            assert None not in st
            ff_len = len(st)
        else:
            st, ff_len = [], 0
        drc = ERR_DATA if any(st) else OK
        corrupt |= drc != 0
        for i, s in zip(cur, st):
            status[i] = s
        unfinished = any(s in (5, 6) for s in st)
        droppable = any(s not in (0, 5, 6) for s in st)
        if not drc or not unfinished or not droppable or r == 3:
            break
        cur = [i for i, s in zip(cur, st) if s in (0, 5, 6)]
    return "%s rc=%d corrupt=%d cur=%s ff=%d status=%s" % (line, rc, int(corrupt), ",".join(map(str, cur)), ff_len, ",".join(map(str, status)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("resident_rules")
    spans = ", ".join('{"%s", %dull, %d, {%s}, {%s}}' % (name, b, len(it), ", ".join("%dull" % p for p, _ in it) or "0", ", ".join("%du" % l for _, l in it) or "0")
                      for name, b, it in SPANS)
    fields = ", ".join("{%d, %du, %du, 0, 0, 0, 0, 0, 0, 0, 0, 0}" % f for f in GROW_FIELDS)
    drops = ", ".join('{"%s", %d, %d, {%s}}' % (name, n, len(rs), ", ".join("{%s}" % ", ".join("-2" if r == "hip" else str(-1 if s is None else s) for s in (r if r != "hip" else [0]))
                                                                           for r in rs) or "{0}") for name, n, rs in DROPS)
    src = d / "probe.cpp"
    src.write_text(PROBE % dict(spans=spans, guesses=", ".join("%dull" % g for g in GUESSES), slots=", ".join("{%du, %du}" % s for s in GROW_SLOTS),
                                fields=fields, drops=drops))
    exe = d / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


def _of(lines, key):
    return [ln[len(key) + 1:] for ln in lines if ln.startswith(key + " ")]


def test_the_method_rules(lines):
    want = ["%d %d %d %d" % (r, s, _methods_ok(r, s), _no_payload(r, s)) for r in range(3) for s in range(3)]
    want += ["-1 0 0 0", "3 1 0 0", "1 3 0 0", "0 -1 0 0"]
    assert _of(lines, "methods") == want


def test_chunk_span_at_its_edges(lines):
    got = _of(lines, "span")
    assert len(got) == len(SPANS)
    for ln, (name, chunk_bytes, items) in zip(got, SPANS):
        rc, b0, e1, bad = _span(chunk_bytes, items)
        msg = "" if bad is None else "who: thing %d lies outside the chunk" % bad
        assert ln == "%s %d %d %d %d|%s" % (name, rc, b0, e1, rc, msg), name
    by = {ln.split()[0]: ln for ln in got}
    assert by["empty"].startswith("empty 0 0 0 ")
    assert by["ends_at_the_end"].startswith("ends_at_the_end 0 16 1000 ") and by["one_byte_past"].startswith("one_byte_past -1 ")
    assert by["pos_past"].startswith("pos_past -1 ") and by["pos_at_the_end"].startswith("pos_at_the_end 0 992 1000 ")
    assert by["wraps"].startswith("wraps -1 ") and by["wraps_inside"].startswith("wraps_inside 0 %d %d " % ((U64 - 100) & ~15, U64 - 1))
    assert by["unaligned"].startswith("unaligned 0 32 701 ") and by["aligned"].startswith("aligned 0 32 64 ")


def test_null_records_are_named(lines):
    assert _of(lines, "records") == ["0 -1|who: record 2 is NULL"]          # (a NULL record of length 0 is an empty record)


def test_the_growth_rule(lines):
    assert _of(lines, "first") == ["%d %d" % (g, min(g, 0xFFFFFF00)) for g in GUESSES]
    got = _of(lines, "grow")
    assert len(got) == 3
    for attempt, ln in enumerate(got):
        retry, bad, slots = _grow(attempt)
        assert ln == "%d %d %d " % (attempt, retry, bad) + " ".join("%d,%d,%d" % s for s in slots), attempt
    first = got[0].split()[3:]
    # status 5 with a reported size: that size; without: eightfold + 64 KiB, the signal slot never below the payload slot; the two clamps
    assert first[0] == "70000,70000,-9" and first[1] == "105536,105536,-9"
    assert first[2] == "%d,%d,-9" % ((8 * 0x0FFFFFFF + 65536,) * 2) and first[3] == "%d,%d,-9" % ((0xFFFFFF00,) * 2) and first[4].startswith("4294967295,")
    assert first[5] == "64,3000,-9" and first[6] == "64,64,-9" and first[7] == "64,64,3"      # status 6; a good record; a corrupt one
    # the attempt limit: after the third attempt nothing grows any more and what is left is bad
    assert got[2].startswith("2 0 1 ") and got[2].split()[3:][0] == "5000,5000,5" and got[2].split()[3:][5] == "64,64,6"
    assert _of(lines, "grow_null") == ["0 1"]


def test_the_dropping_loop_on_a_scripted_decode(lines):
    got = _of(lines, "drop")
    assert len(got) == len(DROPS) and not any("TOO_MANY" in ln for ln in got)
    for ln, (name, n, rounds) in zip(got, DROPS):
        assert ln == name + _drop(n, rounds), name
    by = {ln.split()[0]: ln for ln in got}
    assert by["none"] == "none rc=0 corrupt=0 cur= ff=0 status="
    assert by["all_good"] == "all_good [0,1,2] rc=0 corrupt=0 cur=0,1,2 ff=3 status=0,0,0"
    assert by["corrupt_only"] == "corrupt_only [0,1,2] rc=0 corrupt=1 cur=0,1,2 ff=3 status=0,2,0"
    assert by["unfinished_only"] == "unfinished_only [0,1,2] rc=0 corrupt=1 cur=0,1,2 ff=3 status=0,5,6"
    assert by["corrupt_and_unfinished"] == "corrupt_and_unfinished [0,1,2,3,4] [0,2,3,4] rc=0 corrupt=1 cur=0,2,3,4 ff=4 status=0,3,0,0,0"
    assert by["four_rounds"] == "four_rounds [0,1,2,3,4,5] [1,2,3,4,5] [1,3,4,5] [1,4,5] rc=0 corrupt=1 cur=1,4,5 ff=3 status=2,5,3,4,1,0"
    assert by["hard_error"].startswith("hard_error [0,1,2] [0,2] rc=-2 ")   # any other code of the decode ends the call
