"""bench.py / bench_e2e.py host logic that needs no GPU: the modules import, the traffic stamp only answers for the sources it was collected on, the
e2e helpers pick a directory with room and compare files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_bench_modules_import_and_traffic_stamp_follows_the_sources(tmp_path, monkeypatch):
    import bench
    import bench_e2e  # noqa: F401

    sha = bench.csrc_sha256()
    assert len(sha) == 16
    entries = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    kernels = {e["kernel"] for e in entries}
    assert {"k_encode_stream", "k_inflate_par_np", "k_pack+k_deflate_staged"} <= kernels
    for e in entries:                      # a figure is quoted only for the sources it was measured on
        got, src = bench.pmc_traffic(e["kernel"], e["samples_per_read"], 1000)
        if e["csrc_sha256"] == sha:
            assert got == int(e["hbm_bytes_per_read"] * 1000) and src["csrc_sha256"] == sha
        else:
            assert got is None and src is None
    assert bench.pmc_traffic("no such kernel", 4000, 1) == (None, None)


def test_e2e_helpers(tmp_path):
    import bench_e2e as E

    assert E.pick_dir(1 << 20) in ("/dev/shm", "/tmp")
    assert E.pick_dir(1 << 62) is None
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    a.write_bytes(b"x" * 100000)
    b.write_bytes(b"x" * 100000)
    c.write_bytes(b"x" * 99999 + b"y")
    assert E._same_file(a, b, block=4096) and not E._same_file(a, c, block=4096) and E._same_file(a, a)
    st = E._stamps("s5view[t]    0.232  device ready\nnoise\ns5view[t]    1.674  last write\n")
    assert st == {"device ready": 0.232, "last write": 1.674}


def test_dump_outputs_writes_the_record_stream_as_float_arrays(tmp_path, monkeypatch):
    """--dump-outputs on a host-side stream: lengths and byte sums of every record (across chunk edges), a seeded sample of records
    byte for byte, float .npy only, the same files twice; past DUMP_RECORDS_MAX the per-record arrays are a seeded sample"""
    import numpy as np
    import torch

    import bench

    rng = np.random.default_rng(7)
    lens = rng.integers(9, 400, 3000)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    raw = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    stream = torch.from_numpy(np.concatenate([raw, np.full(64, 7, dtype=np.uint8)]))     # slack past the last record is not output
    rec_off = torch.from_numpy(off)
    d1, d2 = tmp_path / "a", tmp_path / "b"
    got = bench.dump_outputs(str(d1), stream, rec_off, len(lens), chunk=1000)
    bench.dump_outputs(str(d2), stream, rec_off, len(lens))
    names = {"record_index", "record_bytes", "record_byte_sums", "sample_index", "sample_record_bytes"}
    assert set(got["files"]) == names and {p.name for p in d1.iterdir()} == {n + ".npy" for n in names}
    f = {n: np.load(d1 / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in f.values())
    assert sum(a.nbytes for a in f.values()) <= 64 << 20
    assert np.array_equal(f["record_index"], np.arange(len(lens)))
    assert np.array_equal(f["record_bytes"], lens)
    assert np.array_equal(f["record_byte_sums"], [int(raw[off[i]:off[i + 1]].sum(dtype=np.int64)) for i in range(len(lens))])
    pick = f["sample_index"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_RECORDS and (np.diff(pick) > 0).all()
    assert np.array_equal(f["sample_record_bytes"], np.concatenate([raw[off[i]:off[i + 1]] for i in pick]))
    for n in names:
        assert np.array_equal(np.load(d2 / (n + ".npy")), f[n])
    monkeypatch.setattr(bench, "DUMP_RECORDS_MAX", 1000)
    bench.dump_outputs(str(d2), stream, rec_off, len(lens))
    ids = np.load(d2 / "record_index.npy").astype(np.int64)
    assert len(ids) == 1000 and (np.diff(ids) > 0).all()
    assert np.array_equal(np.load(d2 / "record_bytes.npy"), lens[ids])
    assert np.array_equal(np.load(d2 / "record_byte_sums.npy"), f["record_byte_sums"][ids])
