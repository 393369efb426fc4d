"""examples/s5tool.h, what the command-line tools share, held from a small C program of its own (no GPU: the reader runs with `pinned` off,
and nothing else here makes a device call).  The program is built twice, plain and with -fsanitize=address,undefined, and every case runs
under both.

  the chunk reader : BLOW5 files written here (a minimal header, records of chosen sizes with arbitrary bytes: the reader only frames) read
                     with several chunk sizes and K; the framed (file offset, length) list against the file.  Damaged files (no end-of-file
                     marker, a size field past the marker, trailing bytes that make no record, a size above 0xFFFFFF00) give -1 without the
                     buffer growing: s5stats' plain form refused each of them before the reader moved into the header.
  read_reference   : comments, blank lines, CR LF; a bad line by its number; an empty file; 1025 numbers (past the first realloc); the limit.
  xxh64            : against test_digest.xxh64_once.
  rid_layout       : the types s5gpu_aux_types_parse gives, every role `.`; -1 without a `#char*` line.
"""
import os
import struct
import subprocess

import pytest

from test_digest import xxh64_once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "slow5tools_amd")

PROGRAM = r"""
#define _GNU_SOURCE
#define S5TOOL "probe"
#define S5TOOL_DIE 2
#include "s5tool.h"

static int frame(const char *path, size_t chunk, uint32_t K) {
    slow5_file_t *in = slow5_open(path, "r");
    if (!in) return die("cannot open");
    reader_t R;
    if (reader_open(&R, in, path, K, chunk, 0) != 0) {
        printf("open -1\n");
        reader_close(&R);
        slow5_close(in);
        return 0;
    }
    printf("open 0 cap %zu\n", R.cap);
    int64_t n;
    while ((n = next_batch(&R)) > 0) {
        printf("batch %" PRId64 "\n", n);
        for (int64_t i = 0; i < n; i++) {
            uint32_t sum = 0;
            for (uint32_t k = 0; k < R.rec_len[i]; k++) sum += R.buf[R.rec_pos[i] + k];
            printf("rec %" PRIu64 " %u %u\n", file_offset(&R, R.rec_pos[i]), R.rec_len[i], sum);
        }
    }
    printf("end %" PRId64 " cap %zu\n", n, R.cap);
    reader_close(&R);
    slow5_close(in);
    return 0;
}

static int reference(const char *path, size_t most) {
    size_t n = 0;
    float *v = read_reference(path, most, "too many numbers", &n);
    if (!v) { printf("refused\n"); return 0; }
    printf("n %zu\n", n);
    for (size_t i = 0; i < n; i++) printf("%.9g\n", (double)v[i]);
    free(v);
    return 0;
}

static int hash(int argc, char **argv) {
    for (int a = 2; a < argc; a++) {
        const size_t n = (size_t)atol(argv[a]);
        uint8_t *p = (uint8_t *)malloc(n ? n : 1);
        if (!p) return die("out of memory");
        for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(i * 131 + 7);
        printf("%zu %016" PRIx64 "\n", n, xxh64(p, n));
        free(p);
    }
    return 0;
}

static int layout(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return die("cannot open");
    static char text[4096];
    const size_t len = fread(text, 1, sizeof text, f);
    fclose(f);
    s5gpu_skim_layout_t *L = (s5gpu_skim_layout_t *)calloc(1, sizeof *L);
    if (!L) return die("out of memory");
    const int rc = rid_layout(text, len, L);
    printf("rc %d n_aux %u n_unhandled %u\n", rc, L->n_aux, L->n_unhandled);
    for (uint32_t a = 0; rc == 0 && a < L->n_aux; a++) printf("aux %u %d\n", (unsigned)L->type[a], L->role[a] == S5GPU_SKIM_DOT);
    free(L);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 5 && !strcmp(argv[1], "frame")) return frame(argv[2], (size_t)atol(argv[3]), (uint32_t)atol(argv[4]));
    if (argc >= 4 && !strcmp(argv[1], "ref")) return reference(argv[2], (size_t)atol(argv[3]));
    if (argc >= 2 && !strcmp(argv[1], "xxh")) return hash(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "rid")) return layout(argv[2]);
    return 2;
}
"""

TEXT = (b"#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
        b"#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the program, built as the tools are (one gcc line against the built library)"""
    d = tmp_path_factory.mktemp("probe_" + request.param)
    src = d / "probe.c"
    src.write_text(PROGRAM)
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "examples"),
                           str(src), "-o", str(d / "probe"), "-pthread", "-L", HERE, "-lslow5gpu", "-lm", "-Wl,-rpath," + HERE])

    def run(*args):
        p = subprocess.run([str(d / "probe")] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (args, p.returncode, p.stdout[-400:], p.stderr[-2000:])
        return p.stdout.splitlines(), p.stderr

    return run


def blow5(sizes, tail=b"5WOLB", patch=None):
    """a BLOW5 file of records with these sizes; patch = (record, size field to write instead); -> bytes, [(offset of the bytes, size)]"""
    head = bytearray(64)
    head[:6] = b"BLOW5\x01"; head[6:9] = bytes([0, 2, 0]); head[9] = 0; head[10:14] = struct.pack("<I", 1); head[14] = 0
    b = bytes(head) + struct.pack("<I", len(TEXT)) + TEXT
    want = []
    for i, n in enumerate(sizes):
        field = patch[1] if patch and patch[0] == i else n
        want.append((len(b) + 8, n))
        b += struct.pack("<Q", field) + bytes((37 * i + 11 * k + 1) & 255 for k in range(n))
    return b + tail, want


# four records of 8 bytes end at byte 16, 32, 48 and 64 of the record area: exactly at the end of a chunk of 16 and of 64; the records of
# 4000 bytes are larger than those chunks (the buffer grows) and are cut by the end of one of 4096; six records lie whole in the first 4096
# bytes, so K = 3 is reached before the chunk's end
SIZES = [8, 8, 8, 8, 1, 7, 4000, 1, 7, 8, 4000, 7, 1]


@pytest.mark.parametrize("chunk", [16, 64, 4096])
@pytest.mark.parametrize("K", [1, 3, 4096])
def test_reader_frames_every_record_whatever_the_chunk_and_k(probe, tmp_path, chunk, K):
    raw, want = blow5(SIZES)
    path = tmp_path / "a.blow5"
    path.write_bytes(raw)
    out, _ = probe("frame", path, chunk, K)
    assert out[0] == "open 0 cap %d" % chunk
    got = [tuple(int(x) for x in l.split()[1:]) for l in out if l.startswith("rec ")]
    assert [(o, n) for o, n, _ in got] == want
    assert [s for _, _, s in got] == [sum(raw[o:o + n]) for o, n in want]
    batches = [int(l.split()[1]) for l in out if l.startswith("batch ")]
    assert sum(batches) == len(SIZES) and max(batches) <= K
    if K == 1:
        assert batches == [1] * len(SIZES)
    if (chunk, K) == (4096, 3):
        assert batches[:2] == [3, 3]
    end = out[-1].split()
    assert end[:2] == ["end", "0"]
    # the buffer grew for the records of 4000 bytes only: doubled from the chunk until 4008 bytes fit
    cap = chunk
    while cap < 4008:
        cap *= 2
    assert int(end[3]) == cap


def test_reader_trims_the_chunk_for_a_small_file_and_reads_an_empty_one(probe, tmp_path):
    raw, want = blow5([7, 1])
    (tmp_path / "s.blow5").write_bytes(raw)
    out, _ = probe("frame", tmp_path / "s.blow5", 64 << 20, 4096)
    assert out[0] == "open 0 cap %d" % (8 + 7 + 8 + 1 + 4096) and out[1] == "batch 2" and out[-1].split()[:2] == ["end", "0"]
    raw, _ = blow5([])
    (tmp_path / "e.blow5").write_bytes(raw)
    out, _ = probe("frame", tmp_path / "e.blow5", 4096, 3)
    assert out == ["open 0 cap 4096", "end 0 cap 4096"]


DAMAGED = {
    "no end-of-file marker": dict(tail=b""),
    "size field past the marker": dict(patch=(len(SIZES) - 1, 1 + 1000)),
    "size field far past the marker": dict(patch=(4, 100 << 20)),
    "trailing bytes that make no record": dict(tail=b"\x01\x02\x03" + b"5WOLB"),
    "size above 0xFFFFFF00": dict(patch=(4, 0xFFFFFF01)),
    "size above 0xFFFFFF00, first record": dict(patch=(0, 1 << 40)),
}


@pytest.mark.parametrize("what", sorted(DAMAGED))
@pytest.mark.parametrize("chunk", [16, 4096])
def test_reader_refuses_a_damaged_file_without_growing_the_buffer(probe, tmp_path, what, chunk):
    raw, want = blow5(SIZES, **DAMAGED[what])
    path = tmp_path / "d.blow5"
    path.write_bytes(raw)
    out, _ = probe("frame", path, chunk, 3)
    if what == "no end-of-file marker":
        assert out == ["open -1"]
        return
    assert out[0] == "open 0 cap %d" % chunk
    end = out[-1].split()
    print(what, "chunk", chunk, "cap", end[3])
    assert end[:2] == ["end", "-1"]
    # what was framed before the damage is right
    got = [tuple(int(x) for x in l.split()[1:3]) for l in out if l.startswith("rec ")]
    assert got == want[:len(got)]
    # the refusal allocates nothing: the buffer is the chunk, doubled at most until the largest whole record before the damage fits,
    # and so below twice the file
    whole = max([8 + n for _, n in want[:len(got)]] + [0])
    cap = chunk
    while cap < whole:
        cap *= 2
    assert int(end[3]) <= max(cap, chunk) and int(end[3]) <= max(chunk, 2 * len(raw))


def test_read_reference(probe, tmp_path):
    ref = tmp_path / "ref.txt"
    ref.write_bytes(b"# a comment\n\n1.5\r\n-2e3 \n\t\n#x\n0x10\n   7\n3")
    out, err = probe("ref", ref, 100)
    assert out == ["n 5", "1.5", "-2000", "16", "7", "3"] and err == ""
    ref.write_bytes(b"1\n2\n\n# c\nthree\n4\n")
    out, err = probe("ref", ref, 100)
    assert out == ["refused"] and err == "probe: %s line 5 is not a number\n" % ref
    ref.write_bytes(b"1\n2 3\n")
    out, err = probe("ref", ref, 100)
    assert out == ["refused"] and err == "probe: %s line 2 is not a number\n" % ref
    for empty in (b"", b"\n# nothing\n\r\n"):
        ref.write_bytes(empty)
        out, err = probe("ref", ref, 100)
        assert out == ["refused"] and err == "probe: %s holds no number\n" % ref
    ref.write_bytes(b"".join(b"%d.25\n" % i for i in range(1025)))
    out, err = probe("ref", ref, 1025)
    assert out == ["n 1025"] + ["%d.25" % i for i in range(1025)] and err == ""
    out, err = probe("ref", ref, 1024)
    assert out == ["refused"] and err == "probe: %s holds too many numbers\n" % ref
    out, err = probe("ref", tmp_path / "none.txt", 100)
    assert out == ["refused"] and err == "probe: cannot open %s\n" % (tmp_path / "none.txt")


def test_xxh64(probe):
    lengths = [0, 1, 3, 4, 7, 8, 31, 32, 33, 100]
    out, _ = probe("xxh", *lengths)
    assert out == ["%d %016x" % (n, xxh64_once(bytes((i * 131 + 7) & 255 for i in range(n)))) for n in lengths]


def test_rid_layout(probe, tmp_path):
    from slow5tools_amd import ascii

    types = b"#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\tchar*\tdouble\tint32_t\tuint64_t\tuint8_t*\tenum{a,b}"
    text = b"#slow5_version\t0.2.0\n@asic_id\t1\n" + types + b"\n#read_id\tread_group\n"
    (tmp_path / "h.txt").write_bytes(text)
    out, _ = probe("rid", tmp_path / "h.txt")
    want = ascii.aux_types(types)
    assert len(want) == 6
    assert out == ["rc 0 n_aux 6 n_unhandled 6"] + ["aux %d 1" % t for t in want]
    (tmp_path / "h.txt").write_bytes(TEXT)
    out, _ = probe("rid", tmp_path / "h.txt")
    assert out == ["rc 0 n_aux 0 n_unhandled 0"]
    (tmp_path / "h.txt").write_bytes(b"#slow5_version\t0.2.0\n@asic_id\t1\n#read_id\tread_group\n")
    out, _ = probe("rid", tmp_path / "h.txt")
    assert out[0].split()[:2] == ["rc", "-1"]
