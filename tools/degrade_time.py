#!/usr/bin/env python3
"""What degrade's rounding pass costs (k_qts_round).

  degrade_time.py kernel [--reads 1000000] : k_qts_round through s5gpu_qts_round_dev on device-resident signals, timed by device
                                             events (median of 20 launches after 3 warm-ups): 4000-sample reads and one 2 050 027-sample
                                             read.  Bytes moved = 4 per sample (an int16 load and store); share of 6.29 TB/s (the measured
                                             HBM copy rate, MI355X_MICROARCH) beside it.  Run it under `rocprofv3 --kernel-trace --stats`
                                             for the kernel's own time.
  degrade_time.py e2e [--reads 100000]     : whole-process time of `s5view --degrade 3 in out` next to `s5view in out zlib ex-zd` on the
                                             same synthetic zlib + svb-zd file of 4000-sample reads (the two alternate, 3 runs each).
Prints one JSON object per measurement; --out DIR also writes them to DIR/degrade_<mode>.json.
"""
import argparse
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

from slow5tools_amd import _lib, press  # noqa: E402

HBM_TBS = 6.29


def _time_round(L, sig, off, ln, n, bits, reps=20, warm=3):
    st = torch.cuda.current_stream()
    for _ in range(warm):
        _lib.check(L.s5gpu_qts_round_dev(sig.data_ptr(), n, off.data_ptr(), ln.data_ptr(), bits, st.cuda_stream), "s5gpu_qts_round_dev")
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        _lib.check(L.s5gpu_qts_round_dev(sig.data_ptr(), n, off.data_ptr(), ln.data_ptr(), bits, st.cuda_stream), "s5gpu_qts_round_dev")
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def kernel(args):
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    res = []
    for name, n_reads, n in (("4000x%d" % args.reads, args.reads, 4000), ("2050027x1", 1, 2_050_027)):
        stride = (n + 7) // 8 * 8
        sig = torch.randint(-32768, 32767, (n_reads * stride,), dtype=torch.int16, device="cuda")
        off = torch.arange(n_reads, dtype=torch.int64, device="cuda") * stride
        ln = torch.full((n_reads,), n, dtype=torch.int32, device="cuda")
        med, best = _time_round(L, sig, off, ln, n_reads, 3)
        nbytes = 4 * n_reads * n
        r = dict(metric="k_qts_round", shape=name, samples=n_reads * n, bytes=nbytes, event_ms_median=round(med, 4), event_ms_min=round(best, 4),
                 tb_per_s=round(nbytes / (med * 1e-3) / 1e12, 3), frac_of_6_29=round(nbytes / (med * 1e-3) / 1e12 / HBM_TBS, 3))
        print(json.dumps(r), flush=True)
        res.append(r)
        del sig, off, ln
        torch.cuda.empty_cache()
    return res


def _synth_file(path, n_reads, n=4000):
    b = press.DeviceBatch(np.full(n_reads, n, dtype=np.uint64))
    b.synth(); b.encode(); b.compact()
    stream, _ = b.stream_bytes()
    hdr_text = (b"#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
                b"#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n")
    head = bytearray(64)
    head[:6] = b"BLOW5\x01"; head[6:9] = bytes([0, 2, 0]); head[9] = 1; head[10:14] = struct.pack("<I", 1); head[14] = 1
    with open(path, "wb") as f:
        f.write(head); f.write(struct.pack("<I", len(hdr_text))); f.write(hdr_text); f.write(stream); f.write(b"5WOLB")
    del b
    torch.cuda.empty_cache()


def e2e(args):
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    work = args.work or "/tmp"
    src, dst = os.path.join(work, "degrade_in.blow5"), os.path.join(work, "degrade_out.blow5")
    _synth_file(src, args.reads)
    s5view = os.path.join(ROOT, "slow5tools_amd", "s5view")
    cmds = {"view_zlib_exzd": [s5view, src, dst, "zlib", "ex-zd"], "degrade_3": [s5view, "--degrade", "3", src, dst]}
    times = {k: [] for k in cmds}
    for _ in range(3):
        for k, c in cmds.items():
            t = time.perf_counter()
            subprocess.run(c, check=True, capture_output=True, timeout=600)
            times[k].append(time.perf_counter() - t)
    res = []
    for k, v in times.items():
        r = dict(metric="s5view_wall_s", run=k, reads=args.reads, samples_per_read=4000, in_bytes=os.path.getsize(src),
                 wall_s_median=round(float(np.median(v)), 3), wall_s_all=[round(x, 3) for x in v])
        print(json.dumps(r), flush=True)
        res.append(r)
    for p in (src, dst):
        os.remove(p)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--reads", type=int)
    ap.add_argument("--out")
    ap.add_argument("--work")
    a = ap.parse_args()
    if a.reads is None:
        a.reads = 1_000_000 if a.mode == "kernel" else 100_000
    res = kernel(a) if a.mode == "kernel" else e2e(a)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "degrade_%s.json" % a.mode), "w") as f:
            json.dump(res, f, indent=1)
