"""bench.py --dump-outputs: the files hold what the last step computed (here
checked against the oracle's decode of the same seeded wire), in float32 /
float64, whole for a small output and as a seeded sample plus block sums for
a large one, and two runs of the same arguments give the same files."""
import argparse
import importlib.util
import os

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _run_and_dump(b, frames, size, steps, path):
    args = argparse.Namespace(config="c2", frames=frames, size=size, messages=1)
    codec = ca.Codec(0)
    try:
        w = b.Workload(args, codec, 0, torch.device("cuda", 0))
        for _ in range(steps):
            w.step()
        codec.sync()
        files = b.dump_outputs(w, str(path))
        # the wire of the batch the last step decoded, for the oracle
        wire = w.batches[w.turn ^ 1][0].cpu().numpy()
        fs = w.host[1]
        w.close()
    finally:
        codec.close()
    return files, wire, fs


def _load(path, files):
    total = sum(os.path.getsize(os.path.join(str(path), f)) for f in files)
    assert total <= 64 << 20
    return {f[:-4]: np.load(os.path.join(str(path), f)) for f in files}


def test_dump_small_output_whole(tmp_path):
    b = _bench()
    files, wire, fs = _run_and_dump(b, 37, 1000, 3, tmp_path / "a")
    got = _load(tmp_path / "a", files)
    rc, ref, info = oracle.decode_batch(wire, fs)
    assert rc == 0
    assert got["out"].dtype == np.float32 and np.array_equal(got["out"], ref.astype(np.float32))
    for field in ("payload_off", "len", "key", "opcode", "fin", "masked", "hdr_len", "b0", "error"):
        a = got["info_" + field]
        assert a.dtype == np.float64 and np.array_equal(a, info[field].astype(np.float64)), field
    # the same arguments again: the same files, value for value
    files2, _, _ = _run_and_dump(b, 37, 1000, 3, tmp_path / "b")
    again = _load(tmp_path / "b", files2)
    assert sorted(again) == sorted(got)
    assert all(np.array_equal(again[k], got[k]) for k in got)


def test_dump_large_output_sample_and_block_sums(tmp_path):
    b = _bench()
    # 70 x (65536 + 14) B = 4.6 MB: above the whole-file bound, not a multiple of the block
    files, wire, fs = _run_and_dump(b, 70, 65536, 2, tmp_path)
    got = _load(tmp_path, files)
    rc, ref, _ = oracle.decode_batch(wire, fs)
    assert rc == 0 and len(ref) * 4 > b.DUMP_WHOLE_BYTES and len(ref) % b.DUMP_BLOCK != 0
    assert "out" not in got
    pos = np.sort(np.random.default_rng(b.DUMP_SEED).integers(0, len(ref), b.DUMP_SAMPLE))
    assert got["out_sample"].dtype == np.float32 and np.array_equal(got["out_sample"], ref[pos].astype(np.float32))
    whole = len(ref) // b.DUMP_BLOCK * b.DUMP_BLOCK
    sums = np.append(ref[:whole].reshape(-1, b.DUMP_BLOCK).sum(axis=1, dtype=np.int64),
                     ref[whole:].sum(dtype=np.int64))
    assert got["out_block_sums"].dtype == np.float64 and np.array_equal(got["out_block_sums"], sums.astype(np.float64))
