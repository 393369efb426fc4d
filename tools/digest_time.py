#!/usr/bin/env python3
"""What the per-read content digest costs (docs/codecs.md §4.12, k_rec_digest).

  digest_time.py stream [--reads 1000000] : s5gpu_digest_stream on the whole file as ONE chunk (every record in one call), 1 warm-up call and
                                            3 timed ones; prints the call's wall time.  Run it under `rocprofv3 --kernel-trace --stats`
                                            (tools/kstats.sh) for the device time of k_rec_digest beside the decode kernels of the same call.
  digest_time.py mixed [--reads 262144]   : the same call on reads with the lengths of a real run (tools/mixed_lengths.py: log-normal, median
                                            6000 samples, a tail of 50x the median).
  digest_time.py e2e [--reads 1000000]    : whole-process `s5sum in.blow5 > /dev/null` and `s5skim in.blow5 > /dev/null` on the same file, 3 runs
                                            each, alternating: records/s from the first byte read to the last line written.
The file: synthetic reads of 4000 samples, zlib + svb-zd (what s5view writes by default), written to --work (default /dev/shm).
Prints one JSON object per measurement; --out DIR also writes them to DIR/digest_<mode>.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import skim_time  # noqa: E402  (the synthetic file and its framing)
from slow5tools_amd import _lib, press  # noqa: E402


def _time_call(n, raw, pos, lens, what, extra):
    L = _lib.lib()
    dig = np.zeros(n, dtype=np.uint64)
    st = np.zeros(n, dtype=np.int32)
    ts = []
    for k in range(4):
        t = time.perf_counter()
        _lib.check(L.s5gpu_digest_stream(n, raw.ctypes.data, raw.size, pos.ctypes.data, lens.ctypes.data, _lib.REC_ZLIB, _lib.SIG_SVB_ZD,
                                         dig.ctypes.data, st.ctypes.data), "s5gpu_digest_stream")
        if k >= 1:
            ts.append(time.perf_counter() - t)
    assert not st.any() and (dig != 0).all()
    r = dict(metric="s5gpu_digest_stream_wall_s", workload=what, reads=int(n), in_bytes=int(raw.size), wall_s_median=round(float(np.median(ts)), 4),
             wall_s_all=[round(x, 4) for x in ts], records_per_s=round(n / float(np.median(ts))), file_sum="%016x" % (int(dig.sum(dtype=np.uint64)),), **extra)
    print(json.dumps(r), flush=True)
    return [r]


def stream(args, path):
    raw, pos, lens = skim_time._frame(path)
    return _time_call(pos.size, raw, pos, lens, "equal", dict(samples_per_read=4000))


def mixed(args):
    rng = np.random.default_rng(5)
    ns = np.clip(np.exp(rng.normal(np.log(6000), 0.9, args.reads)), 200, 400000).astype(np.uint64)
    b = press.DeviceBatch(ns, rec_method=press.REC_ZLIB, with_stream_out=True)
    tot = b.sig.numel()
    L = _lib.lib()
    # one long synthetic trace cut into the reads (the event model is position-keyed)
    _lib.check(L.s5gpu_synth_dev(b.sig.data_ptr(), 1, tot - 64, tot, 0x5105, 0, b._stream()), "synth")
    _lib.check(L.s5gpu_synth_hdr_dev(b.hdr.data_ptr(), args.reads, 0, b._stream()), "hdr")
    b.encode(); b.compact()
    data, off = b.stream_bytes()
    del b
    torch.cuda.empty_cache()
    raw = np.frombuffer(data + bytes(64), dtype=np.uint8)
    pos = (off[:-1] + 8).astype(np.uint64)
    lens = (off[1:] - off[:-1] - 8).astype(np.uint32)
    return _time_call(args.reads, raw, pos, lens, "mixed", dict(samples_median=int(np.median(ns)), samples_max=int(ns.max()), samples_total=int(ns.sum())))


def e2e(args, path):
    cmds = {"s5sum": [os.path.join(ROOT, "slow5tools_amd", "s5sum"), path], "s5skim": [os.path.join(ROOT, "slow5tools_amd", "s5skim"), path]}
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
        r = dict(metric=k + "_wall_s", reads=args.reads, samples_per_read=4000, in_bytes=os.path.getsize(path), wall_s_median=round(med, 3),
                 wall_s_all=[round(x, 3) for x in v], records_per_s=round(args.reads / med))
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["stream", "mixed", "e2e"])
    ap.add_argument("--reads", type=int)
    ap.add_argument("--out")
    ap.add_argument("--work", default="/dev/shm")
    a = ap.parse_args()
    if a.reads is None:
        a.reads = 262144 if a.mode == "mixed" else 1_000_000
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    if a.mode == "mixed":
        res = mixed(a)
    else:
        src = os.path.join(a.work, "digest_in_%d.blow5" % os.getpid())
        try:
            skim_time._synth_file(src, a.reads)
            res = stream(a, src) if a.mode == "stream" else e2e(a, src)
        finally:
            if os.path.exists(src):
                os.remove(src)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "digest_%s.json" % a.mode), "w") as f:
            json.dump(res, f, indent=1)
