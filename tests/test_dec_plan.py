"""The decode launch layer's rules, without a GPU: csrc/dec_plan.h compiled on its own against the arithmetic the launchers carried inline
before the header existed (csrc/kernels.hip and csrc/host_api.hip of that commit, restated here in Python with the line beside each), on a
grid that sits on every boundary; and the scratch size of the header against the one the built library reports."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slow5tools_amd", "csrc")

REC_NONE, REC_ZLIB, REC_ZSTD = 0, 1, 2
SIG_NONE, SIG_SVB_ZD, SIG_EX_ZD = 0, 1, 2
IP_WAVES, SHORT_PAY, IP_SPAN, NT, ZW_REC = 6, 32768, 4096, 256, 144      # S5_IP_WAVES, S5_IP_SHORT_PAY, inflate_par_dev.h, dev_common.h, zstd_dev.h

# 0 / 1; either side of the svb-zd and of the ex-zd short list; the last valid slot and the first refused one; the largest
MAX_PAY_CAPS = [0, 1, 32768, 32769, 98304, 98305, 0xFFFFFFE0, 0xFFFFFFE1, 2**32 - 1]
MAX_IN_LENS = [0, 1, 4000, 4001]
# 1; either side of: the weights pass, routing, the order list, k_inflate_long's grid, the lane family, the fallback's grid, k_unpack_rest's grid
N_RECS = [1, 255, 256, 1023, 1024, 8191, 8192, 16384, 16385, 24575, 24576, 262144, 262145, 524288, 524289]
RESIDENT = [1, 1000, 6144]
UNPACK_FUSED, INFLATE_PAR, INFLATE_ROUTE, NP_LDS_PAYLOAD = [0, 1], [0, 1, 2], [0, 1], [0, 1]
ORDER_MIN, ZSTD_PRE_MIN, INFLATE_SIMT_MIN = [0, 8192], [0, 256], [0, 24576]


def _slot(cap):
    """kernels.hip:2157 (s5gpu_decode_scratch_bytes), :2193 (s5gpu_decode_dev), host_api.hip:1025 (decode_np_framed)"""
    return (cap + 16 + 15) & ~15


def _scratch_bytes(cap):
    """kernels.hip:2158"""
    return 64 + _slot(cap) * (256 * IP_WAVES * 4 + 256)


def _payload_bytes(cap):
    """for a slot s: either side of the two-slot floor; 16 and 32 slots (n_fb 1 and 2); 4096 and 4112 (either side of n_fb = 256: 4096 slots give
    256 already); what s5gpu_decode_scratch_bytes names"""
    s = _slot(cap)
    return [64 + 2 * s - 1, 64 + 2 * s, 64 + 16 * s, 64 + 32 * s, 64 + 4096 * s, 64 + 4112 * s, _scratch_bytes(cap)]


PROBE = r"""
#include <stdio.h>
#include "dec_plan.h"
using namespace s5plan;
typedef unsigned long long ull;
int main() {
    const uint32_t caps[] = {%(caps)s};
    const uint32_t in_lens[] = {%(in_lens)s};
    const uint32_t recs[] = {%(recs)s};
    const uint32_t resident[] = {%(resident)s};
    const uint32_t order_min[] = {%(order_min)s}, pre_min[] = {%(pre_min)s}, simt_min[] = {%(simt_min)s};
    printf("const %%u %%u %%u %%u %%u\n", IP_WAVES, SHORT_PAY, IP_SPAN, WG, ZW_WORDS);
    for (int r = 0; r < 3; r++)
        for (int s = 0; s < 3; s++) {
            printf("served %%d %%d %%d\n", r, s, (int)np_served(r, s));
            for (uint32_t uf = 0; uf < 2; uf++)
                for (uint32_t ip = 0; ip < 3; ip++) printf("fused %%d %%d %%u %%u %%d\n", r, s, uf, ip, fused_unpack(r, s, uf, ip));
            for (uint32_t c : caps)
                for (uint32_t l : in_lens)
                    for (uint32_t o = 0; o < 2; o++) {
                        printf("variant %%d %%d %%u %%u %%u ", r, s, c, l, o);
                        if (c) printf("%%d\n", np_variant(r, s, c, l, o)); else printf("-\n");     // (max_pay_cap 0 is refused before a variant is chosen)
                    }
        }
    for (uint32_t c : caps) {
        printf("cap %%u %%d %%d %%d %%llu %%llu\n", c, (int)short_list(0, c), (int)short_list(1, c), (int)short_list(2, c), (ull)np_slot(c), (ull)np_scratch_bytes(c));
        for (uint32_t n : recs) printf("host %%u %%u %%llu\n", c, n, (ull)np_scratch_for(np_scratch_bytes(c), c, n));
        const uint64_t s = np_slot(c);
        const uint64_t pbs[] = {64 + 2 * s - 1, 64 + 2 * s, 64 + 16 * s, 64 + 32 * s, 64 + 4096 * s, 64 + 4112 * s, np_scratch_bytes(c)};
        for (uint64_t pb : pbs) {
            printf("args %%u %%llu %%d\n", c, (ull)pb, (int)np_args_ok(c, pb));
            if (!np_args_ok(c, pb)) continue;
            for (int r = 0; r < 3; r++)
                for (uint32_t res : resident)
                    for (uint32_t n : recs) {
                        const NpShape h = np_shape(r, c, pb, res, n);
                        printf("shape %%d %%u %%llu %%u %%u %%llu %%llu %%llu %%d\n", r, c, (ull)pb, res, n, (ull)h.n_slots, (ull)h.n_fb, (ull)h.n_main, (int)h.ticket);
                    }
        }
    }
    for (uint32_t n : recs) {
        printf("grids %%u %%u %%u %%u %%u\n", n, fallback_grid(n), unpack_rest_grid(n), long_grid(n), lane_grid(n));
        for (uint32_t o = 0; o < 2; o++) printf("routed %%u %%u %%d\n", n, o, (int)lane_routed(n, o));
        for (uint32_t m : order_min) printf("order %%u %%u %%d\n", n, m, (int)from_count(n, m));
        for (uint32_t m : pre_min) printf("pre %%u %%u %%llu\n", n, m, (ull)zstd_pre_words(n, m));
        for (int r = 0; r < 3; r++)
            for (uint32_t ip = 0; ip < 3; ip++)
                for (uint32_t m : simt_min) printf("family %%d %%u %%u %%u %%d %%d\n", r, n, ip, m, (int)inflate_family(r, n, ip, m), (int)par_fallback(ip));
    }
    return 0;
}
"""


def _short_list(sig, cap):
    """kernels.hip:2061 (launch_inflate); :2204 is the same without the first test, behind a max_pay_cap that :2194 has refused when 0"""
    return int(cap != 0 and cap <= SHORT_PAY * (3 if sig == SIG_EX_ZD else 1))


def _served(rec, sig):
    """kernels.hip:2188-2189, and resident_rules.h:21 (decodes_without_payload)"""
    np_xz = sig == SIG_EX_ZD and rec == REC_ZLIB
    return int(not (not np_xz and (sig != SIG_SVB_ZD or (rec != REC_ZLIB and rec != REC_ZSTD))))


def _args_ok(cap, payload_bytes):
    """kernels.hip:2194"""
    slot = _slot(cap)
    return int(not (cap == 0 or slot > 0xFFFFFFF0 or payload_bytes < 64 + 2 * slot))


def _variant(rec, sig, cap, max_in_len, np_lds_payload):
    """kernels.hip:2188, :2199, :2204, :2208-2209"""
    np_xz = sig == SIG_EX_ZD and rec == REC_ZLIB
    zl = rec == REC_ZLIB
    shortrec_np = cap <= SHORT_PAY * (3 if np_xz else 1)
    lds_pay = zl and not np_xz and np_lds_payload and max_in_len != 0 and max_in_len <= IP_SPAN - 96
    return 4 if not zl else 5 if lds_pay else (2 if np_xz else 0) + (1 if shortrec_np else 0)


def _shape(rec, cap, payload_bytes, resident, n_recs):
    """kernels.hip:2198-2201, :2220-2221, :2230"""
    n_slots = (payload_bytes - 64) // _slot(cap)
    zl = rec == REC_ZLIB
    n_fb = (1 if n_slots // 16 < 1 else 256 if n_slots // 16 > 256 else n_slots // 16) if zl else 0
    n_main = min(n_slots - n_fb, resident, n_recs)
    ticket = not (zl and n_recs <= n_main)
    return n_slots, n_fb, n_main, int(ticket)


def _host_scratch(cap, n):
    """host_api.hip:1025-1030 (decode_np_framed)"""
    slot = _slot(cap)
    scratch = _scratch_bytes(cap)
    enough, floor_, ceil_ = 64 + slot * (n + 257), 64 + 2 * slot, 1 << 30
    scratch = min(scratch, enough)
    scratch = min(scratch, ceil_)
    return max(scratch, floor_)


def _fused(rec, sig, unpack_fused, inflate_par):
    """kernels.hip:2251-2253"""
    rec_ok = (rec == REC_ZLIB and inflate_par == 1) or rec == REC_ZSTD
    return 0 if not unpack_fused else 1 if sig == SIG_SVB_ZD and rec_ok else 2 if sig == SIG_EX_ZD and rec_ok else 0


def _family(rec, n, inflate_par, simt_min):
    """kernels.hip:2048, :2055, :2067, :2094: zstd 0, parallel 1, lane 2, wave 3; the fallback pass of :2066"""
    fam = 0 if rec == REC_ZSTD else 1 if rec == REC_ZLIB and inflate_par else 2 if rec == REC_ZLIB and n >= simt_min else 3
    return fam, int(inflate_par == 1)


def _u32(x):
    return x & 0xFFFFFFFF


def _grids(n):
    """kernels.hip:2065 (fallback), :2258 (k_unpack_rest), :2089 (k_inflate_long), :2053 (weights pass); n_recs is a uint32_t"""
    return min(_u32(n + 63) // 64, 4096), min(_u32(n + NT - 1) // NT, 2048), min(n, 16384), _u32(n + 63) // 64


def _want():
    w = ["const %d %d %d %d %d" % (IP_WAVES, SHORT_PAY, IP_SPAN, NT, ZW_REC // 4)]
    for r in range(3):
        for s in range(3):
            w.append("served %d %d %d" % (r, s, _served(r, s)))
            w += ["fused %d %d %d %d %d" % (r, s, uf, ip, _fused(r, s, uf, ip)) for uf in UNPACK_FUSED for ip in INFLATE_PAR]
            w += ["variant %d %d %d %d %d %s" % (r, s, c, l, o, _variant(r, s, c, l, o) if c else "-")
                  for c in MAX_PAY_CAPS for l in MAX_IN_LENS for o in NP_LDS_PAYLOAD]
    for c in MAX_PAY_CAPS:
        w.append("cap %d %d %d %d %d %d" % (c, _short_list(0, c), _short_list(1, c), _short_list(2, c), _slot(c), _scratch_bytes(c)))
        w += ["host %d %d %d" % (c, n, _host_scratch(c, n)) for n in N_RECS]
        for pb in _payload_bytes(c):
            w.append("args %d %d %d" % (c, pb, _args_ok(c, pb)))
            if _args_ok(c, pb):
                w += ["shape %d %d %d %d %d %d %d %d %d" % ((r, c, pb, res, n) + _shape(r, c, pb, res, n)) for r in range(3) for res in RESIDENT for n in N_RECS]
    for n in N_RECS:
        w.append("grids %d %d %d %d %d" % ((n,) + _grids(n)))
        w += ["routed %d %d %d" % (n, o, int(n >= 1024 and bool(o))) for o in INFLATE_ROUTE]                       # kernels.hip:2074
        w += ["order %d %d %d" % (n, m, int(bool(m) and n >= m)) for m in ORDER_MIN]                                 # kernels.hip:1704, :1715
        w += ["pre %d %d %d" % (n, m, n * (ZW_REC // 4) if m and n >= m else 0) for m in ZSTD_PRE_MIN]               # kernels.hip:1711
        w += ["family %d %d %d %d %d %d" % ((r, n, ip, m) + _family(r, n, ip, m)) for r in range(3) for ip in INFLATE_PAR for m in INFLATE_SIMT_MIN]
    return w


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("dec_plan")
    src = d / "probe.cpp"
    u = lambda xs: ", ".join("%uu" % x for x in xs)
    src.write_text(PROBE % dict(caps=u(MAX_PAY_CAPS), in_lens=u(MAX_IN_LENS), recs=u(N_RECS), resident=u(RESIDENT), order_min=u(ORDER_MIN),
                                pre_min=u(ZSTD_PRE_MIN), simt_min=u(INFLATE_SIMT_MIN)))
    exe = d / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


def test_decode_rules_equal_the_launchers_arithmetic(plan_lines):
    want = _want()
    assert len(plan_lines) == len(want)
    for g, w in zip(plan_lines, want):
        assert g == w


def test_the_grid_reaches_every_branch(plan_lines):
    """every variant, both sides of every yes / no rule, the three values of the fallback count's clamp and a refused slot are in the lines compared"""
    kinds = {}
    for ln in plan_lines:
        f = ln.split()
        kinds.setdefault(f[0], set()).add(tuple(f[1:]))
    assert {f[-1] for f in kinds["variant"]} == {"-", "0", "1", "2", "3", "4", "5"}
    assert {f[-1] for f in kinds["fused"]} == {"0", "1", "2"}
    assert {f[-2] for f in kinds["family"]} == {"0", "1", "2", "3"}
    assert {f[-1] for f in kinds["args"]} == {"0", "1"} and ("4294967265", str(_scratch_bytes(0xFFFFFFE1)), "0") in kinds["args"]
    assert {f[-1] for f in kinds["shape"]} == {"0", "1"}                           # the ticket counter
    assert {"1", "2", "256"} <= {f[-3] for f in kinds["shape"] if f[0] == "1"} and {f[-3] for f in kinds["shape"] if f[0] != "1"} == {"0"}     # n_fb
    for k in ("served", "routed", "order"):
        assert {f[-1] for f in kinds[k]} == {"0", "1"}


def test_scratch_bytes_of_the_header_is_what_the_library_reports(plan_lines):
    from slow5tools_amd import _lib

    L = _lib.lib()           # (loads without a GPU: no device is touched)
    L.s5gpu_decode_scratch_bytes.restype = ctypes.c_uint64
    L.s5gpu_decode_scratch_bytes.argtypes = [ctypes.c_uint32]
    header = {int(f[1]): int(f[6]) for f in (ln.split() for ln in plan_lines) if f[0] == "cap"}
    assert sorted(header) == sorted(MAX_PAY_CAPS)
    for c in MAX_PAY_CAPS:
        assert int(L.s5gpu_decode_scratch_bytes(c)) == header[c] == _scratch_bytes(c)
