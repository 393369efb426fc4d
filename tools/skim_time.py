#!/usr/bin/env python3
"""What skim costs (docs/codecs.md §4.9, k_skim_format).

  skim_time.py kernel [--reads 1000000] : s5gpu_skim_stream on the whole file as ONE chunk (every record in one call), 3 warm-up calls and
                                          5 timed ones; prints the call's wall time.  Run it under `rocprofv3 --kernel-trace --stats`
                                          (tools/kstats.sh) for the device time split into the inflate kernels and k_skim_format.
  skim_time.py e2e [--reads 1000000]    : whole-process `s5skim in.blow5 > /dev/null` on the same file, default -K (4096) and -K 65536,
                                          3 runs each, alternating: records/s from the first byte read to the last line written.
The file: synthetic reads of 4000 samples, zlib + svb-zd (what s5view writes by default), written to --work (default /dev/shm).
Prints one JSON object per measurement; --out DIR also writes them to DIR/skim_<mode>.json.
"""
import argparse
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib, press, skim  # noqa: E402

HDR_TEXT = (b"#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
            b"#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n")


def _synth_file(path, n_reads, n=4000, piece=250_000):
    head = bytearray(64)
    head[:6] = b"BLOW5\x01"; head[6:9] = bytes([0, 2, 0]); head[9] = 1; head[10:14] = struct.pack("<I", 1); head[14] = 1
    with open(path, "wb") as f:
        f.write(head); f.write(struct.pack("<I", len(HDR_TEXT))); f.write(HDR_TEXT)
        for first in range(0, n_reads, piece):
            m = min(piece, n_reads - first)
            b = press.DeviceBatch(np.full(m, n, dtype=np.uint64))
            b.synth(first=first); b.encode(); b.compact()
            stream, _ = b.stream_bytes()
            f.write(stream)
            del b
            torch.cuda.empty_cache()
        f.write(b"5WOLB")


def _frame(path):
    raw = np.fromfile(path, dtype=np.uint8)
    (hl,) = struct.unpack_from("<I", raw[64:68].tobytes())
    p, end, pos, lens = 68 + hl, raw.size - 5, [], []
    while p < end:
        (sz,) = struct.unpack_from("<Q", raw[p : p + 8].tobytes())
        pos.append(p + 8); lens.append(sz)
        p += 8 + sz
    return raw, np.array(pos, dtype=np.uint64), np.array(lens, dtype=np.uint32)


def kernel(args, path):
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    raw, pos, lens = _frame(path)
    n = pos.size
    lay = skim.layout(HDR_TEXT)
    cap = 160 * n + 4096
    out = np.empty(cap, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    ts = []
    for k in range(8):
        t = time.perf_counter()
        _lib.check(L.s5gpu_skim_stream(n, raw.ctypes.data, raw.size, pos.ctypes.data, lens.ctypes.data, _lib.REC_ZLIB, _lib.SIG_SVB_ZD, C.byref(lay),
                                       out.ctypes.data, cap, off.ctypes.data, None), "s5gpu_skim_stream")
        if k >= 3:
            ts.append(time.perf_counter() - t)
    r = dict(metric="s5gpu_skim_stream_wall_s", reads=int(n), samples_per_read=4000, in_bytes=int(raw.size), out_bytes=int(off[n]),
             wall_s_median=round(float(np.median(ts)), 4), wall_s_all=[round(x, 4) for x in ts], records_per_s=round(n / float(np.median(ts))))
    print(json.dumps(r), flush=True)
    return [r]


def e2e(args, path):
    s5skim = os.path.join(ROOT, "slow5tools_amd", "s5skim")
    cmds = {"K4096": [s5skim, path], "K65536": [s5skim, "-K", "65536", path]}
    times = {k: [] for k in cmds}
    for _ in range(3):
        for k, c in cmds.items():
            with open(os.devnull, "wb") as dn:
                t = time.perf_counter()
                subprocess.run(c, check=True, stdout=dn, timeout=900)
                times[k].append(time.perf_counter() - t)
    res = []
    for k, v in times.items():
        med = float(np.median(v))
        r = dict(metric="s5skim_wall_s", run=k, reads=args.reads, samples_per_read=4000, in_bytes=os.path.getsize(path),
                 wall_s_median=round(med, 3), wall_s_all=[round(x, 3) for x in v], records_per_s=round(args.reads / med))
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--out")
    ap.add_argument("--work", default="/dev/shm")
    a = ap.parse_args()
    src = os.path.join(a.work, "skim_in_%d.blow5" % os.getpid())
    try:
        _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
        _synth_file(src, a.reads)
        res = kernel(a, src) if a.mode == "kernel" else e2e(a, src)
    finally:
        if os.path.exists(src):
            os.remove(src)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "skim_%s.json" % a.mode), "w") as f:
            json.dump(res, f, indent=1)
