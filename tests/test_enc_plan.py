"""The encode launch layer's rules, without a GPU: csrc/enc_plan.h compiled on its own against the arithmetic the launchers carried
before the header existed (restated here in Python), and the option table of s5gpu_set_option at its bounds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slow5tools_amd", "csrc")

BLK = 16384                      # DEFL_BLK
SIG_NONE, SIG_SVB_ZD, SIG_EX_ZD = 0, 1, 2
LDS_CAPS = [0, 1, 2048, 8192, 8193, 16384, 70000]
# payload bounds: tiny ones; 4000 and 6400 samples with a 74-byte head (svb-zd 13086 / 20886, ex-zd 38106 / 60906); either side of a cap of
# exactly 8192 (svb-zd 16909 / 16910); around 65536 * 4 * 3.25; each method's own first "long" bound and the one below it; the largest
MAX_PAYLOADS = [0, 1, 15, 86, 13086, 16909, 16910, 20886, 38106, 60906, 851967, 851968, 851969, 2**32 - 1,
                65536, 65537, 212995, 212996, 622601, 622602]
GROUPS = [1, 4]                  # svb-zd blobs per workgroup: s5gpu_svbzd_encode_dev, s5gpu_svbzd_encode_stream_dev

PROBE = r"""
#include <stdio.h>
#include "enc_plan.h"
int main() {
    const int sigs[] = {%(sigs)s};
    const uint32_t caps[] = {%(caps)s};
    const uint32_t pays[] = {%(pays)s};
    const uint32_t groups[] = {%(groups)s};
    printf("%%u %%u %%u %%.17g %%.17g %%.17g\n", s5plan::BLK, s5plan::MIXED_BUDGET, s5plan::NARROW_MAX, s5plan::fit_per_sample(0),
           s5plan::fit_per_sample(1), s5plan::fit_per_sample(2));
    for (int s : sigs)
        for (uint32_t c : caps)
            for (uint32_t m : pays) {
                const uint32_t cap = s5plan::fused_cap(s, m, c, s5plan::BLK);
                printf("%%d %%u %%u %%u %%d %%d %%d", s, c, m, cap, (int)s5plan::all_staged(s, m, c, s5plan::BLK), (int)s5plan::wide(cap),
                       (int)s5plan::batch_is_long(s, m, s5plan::BLK));
                for (uint32_t g : groups) printf(" %%u", s5plan::svb_blob_cap(m, c, g));
                printf("\n");
            }
    return 0;
}
"""


def _u32(x):
    return x & 0xFFFFFFFF


def _fused_cap(sig, max_payload, lds_cap):
    """s5gpu_encode_dev / fused_cap() before enc_plan.h"""
    cap = lds_cap
    if cap == 0:
        if sig == SIG_SVB_ZD:
            cap = _u32(_u32(max_payload * 155 // 325) + 128)
        elif sig == SIG_EX_ZD:
            cap = _u32(_u32(max_payload * 130 // 950) + 256)
        else:
            cap = max_payload
    cap = min(cap, max_payload, BLK)
    return _u32(cap + 15) & ~15


def _is_long(sig, max_payload):
    """host_api.hip's encode_batch_one, and the staged test of s5gpu_encode_dev"""
    div = 325 if sig == SIG_SVB_ZD else 950 if sig == SIG_EX_ZD else 100
    return max_payload * 100 // div > 4 * 16384


def _blob_cap(max_payload, lds_cap, group):
    """s5gpu_svbzd_encode_dev (group 1) / s5gpu_svbzd_encode_stream_dev (group 4)"""
    cap = lds_cap if lds_cap else max_payload * 155 // 325 + 128
    cap = min(cap * group, 64 * 1024)
    return (cap + 15) & ~15


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("enc_plan")
    src = d / "probe.cpp"
    src.write_text(PROBE % dict(sigs=", ".join(map(str, (SIG_NONE, SIG_SVB_ZD, SIG_EX_ZD))), caps=", ".join("%uu" % c for c in LDS_CAPS),
                                pays=", ".join("%uu" % m for m in MAX_PAYLOADS), groups=", ".join("%uu" % g for g in GROUPS)))
    exe = d / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


def test_header_constants(plan_lines):
    blk, mixed, narrow, per_none, per_svb, per_exzd = plan_lines[0].split()
    assert (int(blk), int(mixed), int(narrow)) == (BLK, 8192, 8192)
    assert (float(per_none), float(per_svb), float(per_exzd)) == (2.0, 1.55, 1.30)      # the very doubles of the host layer's fit count


def test_budget_rules_equal_the_launchers_arithmetic(plan_lines):
    want = []
    for s in (SIG_NONE, SIG_SVB_ZD, SIG_EX_ZD):
        for c in LDS_CAPS:
            for m in MAX_PAYLOADS:
                cap = _fused_cap(s, m, c)
                row = [s, c, m, cap, int(c == 0 and _is_long(s, m)), int(cap > 8192), int(_is_long(s, m))] + [_blob_cap(m, c, g) for g in GROUPS]
                want.append(" ".join(map(str, row)))
    got = plan_lines[1:]
    assert len(got) == len(want) == 3 * len(LDS_CAPS) * len(MAX_PAYLOADS)
    for g, w in zip(got, want):
        assert g == w


@pytest.mark.parametrize("sig,n,cap,wide", [(SIG_SVB_ZD, 4000, 6384, False), (SIG_SVB_ZD, 6400, 10096, True),
                                            (SIG_EX_ZD, 4000, 5472, False), (SIG_EX_ZD, 6400, 8592, True)])
def test_budgets_of_the_four_stream_kernel_shapes(plan_lines, sig, n, cap, wide):
    """4000 and 6400 samples behind a 74-byte head: the narrow and the wide variant of either signal method"""
    sigb = 4 + (n + 3) // 4 + 3 * n if sig == SIG_SVB_ZD else 24 + 2 * ((n + 3) // 4 + 4 * n) + n
    pay = 74 + 8 + sigb
    row = [ln.split() for ln in plan_lines[1:] if ln.startswith("%d 0 %d " % (sig, pay))]
    assert len(row) == 1
    assert (int(row[0][3]), int(row[0][4]), int(row[0][5])) == (cap, 0, int(wide))


# name: (lowest, highest or None for "no upper bound", default)
OPTIONS = {
    "inflate_simt_min": (0, None, 24576),
    "inflate_route": (0, 1, 1),
    "np_lds_payload": (0, 1, 1),
    "fused_tier2": (0, 16384, 0),
    "zstd_sequences": (0, 1, 1),
    "unpack_fused": (0, 1, 1),
    "inflate_par": (0, 2, 1),
    "zstd_pre_min": (0, None, 256),
    "order_min": (0, None, 8192),
}


def test_option_table_accepts_its_ranges_and_nothing_else():
    from slow5tools_amd import _lib

    L = _lib.lib()           # (loads without a GPU: no device is touched by an option)
    OK, ERR_ARG = 0, -1
    try:
        for name, (lo, hi, _) in OPTIONS.items():
            key = name.encode()
            assert L.s5gpu_set_option(key, lo) == OK, name
            assert L.s5gpu_set_option(key, hi if hi is not None else 2**31 - 1) == OK, name
            assert L.s5gpu_set_option(key, lo - 1) == ERR_ARG, name
            assert L.s5gpu_last_error() == b"s5gpu_set_option: unknown option"
            if hi is not None:
                assert L.s5gpu_set_option(key, hi + 1) == ERR_ARG, name
        assert L.s5gpu_set_option(b"fused_tier2", 16385) == ERR_ARG
        assert L.s5gpu_set_option(b"fused_tier2", 12300) == OK          # (kept in 16-byte units: 12288)
        assert L.s5gpu_set_option(b"no_such_option", 1) == ERR_ARG
        assert L.s5gpu_last_error() == b"s5gpu_set_option: unknown option"
        assert L.s5gpu_set_option(None, 1) == ERR_ARG
    finally:
        for name, (_, _, default) in OPTIONS.items():
            assert L.s5gpu_set_option(name.encode(), default) == OK
