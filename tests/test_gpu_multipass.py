"""Second and later passes of the batch kernels' loops against the oracle.

At the sizes of the other tests every k_decode block handles one tile and one
slice of frames, and the piece path's scan of scan-block sums runs once.  Here
`$WSG_DEC_BLOCKS_PER_CU` caps the decode grid so that a wire of ~13 MiB gives
every block up to four tiles of different paths in turn (staged tiles of
several rounds, stream and boundary tiles, staged tiles of one round, the
wire's partial last tile), and a ragged batch of more than 2 x 262 144 frames
takes the piece path's carry loop through three passes.  Every test first
asserts that its input reaches the pass it is for, from the device's CU count.
Bit-exact, no tolerance.
"""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import workloads as wl  # noqa: E402
from cppserver_amd.layout import RECV_INFO, SEND_DESC, frame_sizes  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402
from tests.test_gpu_parity import INFO_FIELDS, SMALL_AVG, _mixed_desc  # noqa: E402

TILE = 16384            # wsg_internal.h: bytes of one k_decode tile
BLOCK = 256             # ... threads of a block: frames of one info slice
SCAN_ITEMS = 1024       # ... frames of one encode scan block
DEC_BLOCKS_PER_CU = 4096   # the default k_decode grid cap
SENTINEL = 0xA5
PAD = 4096              # sentinel bytes behind every output


@pytest.fixture(scope="module")
def codecs():
    """per_cu -> a context whose decode grid is capped at that many blocks per CU (None: the default)."""
    made = {}

    def get(per_cu=None):
        if per_cu not in made:
            made[per_cu] = _codec() if per_cu is None else _codec(WSG_DEC_BLOCKS_PER_CU=per_cu)
        return made[per_cu]

    yield get
    for c in made.values():
        c.close()


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _grid(tiles, n, per_cu):
    """k_decode's grid as decode_launch sizes it."""
    return max(1, min(max(tiles, -(-n // BLOCK)), _cus() * per_cu))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ the wire
def _region(rng, lo, hi, nbytes):
    """Descriptors of frames with payloads of lo..hi bytes, about nbytes of wire."""
    count = int(nbytes // ((lo + hi) // 2 + 4)) * 2 + 16
    desc = np.zeros(count, dtype=SEND_DESC)
    desc["len"] = rng.integers(lo, hi + 1, count)
    desc["opcode"] = rng.choice([0x81, 0x82, 0x01, 0x02, 0x00, 0x80, 0x89, 0x8A, 0xC2, 0x83], count)
    desc["mask"] = rng.random(count) < 0.6
    desc["key"] = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    desc["src_off"] = rng.integers(0, 4096, count)
    keep = int(np.searchsorted(np.cumsum(frame_sizes(desc)), nbytes)) + 1
    assert keep < count
    return desc[:keep]


@functools.lru_cache(maxsize=None)
def _wire(order):
    """(wire, frame starts, region byte ranges by name, oracle's rc/out/info).
    Regions of about G = CUs tiles each, so that with a grid of G blocks one
    block meets each region's tile path in turn:
      R0 payloads 0-20 B: staged tiles of several rounds (and > 256 G frames)
      R1 60 000-200 000 B: stream and boundary tiles
      R2 100-3 000 B: staged tiles of one round
      R3 0.3 G tiles of R0's kind, the wire ending off a 16-byte boundary."""
    g = _cus()
    rng = np.random.default_rng(20 + len(order) + order.index("R0"))
    spec = {"R0": (0, 20, g * TILE), "R1": (60000, 200000, g * TILE), "R2": (100, 3000, g * TILE),
            "R3": (0, 20, 3 * g * TILE // 10)}
    parts = [_region(rng, *spec[name]) for name in order]
    desc = np.concatenate(parts)
    if int(frame_sizes(desc).sum()) % 16 == 0:
        desc["len"][-1] += 1 if desc["len"][-1] < 20 else -1
    payload = wl.random_bytes(rng, 4096 + 200000 + 16)
    wire, off = oracle.encode_batch(payload, desc)
    assert len(wire) % 16 != 0
    bounds = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    regions = {name: (int(off[bounds[k]]), int(off[bounds[k + 1]])) for k, name in enumerate(order)}
    fs = off[:-1].copy()
    return wire, fs, regions, oracle.decode_batch(wire, fs)


ORDERS = [("R0", "R1", "R2", "R3"), ("R2", "R1", "R0", "R3")]


def _assert_strides(wire_len, n, per_cu):
    """The batch makes a grid of per_cu blocks per CU stride: tiles and info slices."""
    tiles = -(-wire_len // TILE)
    grid = _grid(tiles, n, per_cu)
    assert grid == _cus() * per_cu
    if per_cu == 1:
        assert tiles > 3 * grid            # every block: three tiles, some a fourth
    else:
        assert grid < tiles < 2 * grid     # some blocks two tiles, some one
    assert n > grid * BLOCK                # the per-frame info slice strides too
    assert wire_len % TILE != 0 and (tiles - 1) >= grid   # the partial last tile is a later pass of its block
    return grid


def _check(got_rc, got_out, got_info, ref):
    rc_o, out_o, info_o = ref
    assert got_rc == rc_o
    assert np.array_equal(got_out, out_o)
    for f in INFO_FIELDS:
        assert np.array_equal(got_info[f], info_o[f]), f


def _decode(codec, wire, fs, inplace, prepared=False):
    """Device decode of `wire` into exactly len(wire) bytes of a sentinel-filled
    buffer (in place: the wire sits in that buffer); the sentinel behind the
    output and behind the records must survive."""
    n, nbytes = len(fs), len(wire)
    buf = torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    ibuf = torch.full((n * RECV_INFO.itemsize + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[:nbytes]
    if inplace:
        out.copy_(torch.from_numpy(np.asarray(wire)))
        w = out
    else:
        w = dev(wire)
    f = dev(np.asarray(fs).view(np.int64))
    if prepared:
        codec.prepare_decode(w, f, out, ibuf)()
    else:
        codec.decode_batch(w, f, out=out, info=ibuf)
    rc = codec.sync_status()
    assert bool((buf[nbytes:] == SENTINEL).all()), "bytes written past wire_len"
    assert bool((ibuf[n * RECV_INFO.itemsize:] == SENTINEL).all()), "records written past frame n"
    return rc, out.cpu().numpy(), ca.info_to_numpy(ibuf, n)


# ------------------------------------------------- k_decode, tiles per block
@pytest.mark.parametrize("per_cu", [1, 3])
@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "".join(o))
def test_decode_several_tiles_per_block(codecs, order, per_cu):
    """Block b of a G-block grid takes tiles b, b + G, b + 2G, b + 3G: one
    tile path after another in the same block (the staged path's LDS arrays
    and its first barrier reused across tiles), and the per-frame info slice
    over several passes.  Out of place and in place."""
    wire, fs, _, ref = _wire(order)
    _assert_strides(len(wire), len(fs), per_cu)
    assert ref[0] == 0
    c = codecs(per_cu)
    for inplace in (False, True):
        _check(*_decode(c, wire, fs, inplace), ref)


def test_decode_several_tiles_prepared_and_host(codecs):
    """The same wire through prepare_decode's bound launch and through the
    staged host pipeline (pageable buffers): the slot's segment strides too."""
    wire, fs, _, ref = _wire(ORDERS[0])
    _assert_strides(len(wire), len(fs), 1)
    c = codecs(1)
    _check(*_decode(c, wire, fs, False, prepared=True), ref)
    pageable = np.array(wire)
    out = np.full(len(wire) + PAD, SENTINEL, dtype=np.uint8)
    rc, got, info = c.decode_batch_host(pageable, np.array(fs), out=out)
    _check(rc, got, info, ref)
    assert (out[len(wire):] == SENTINEL).all()


def test_decode_errors_from_later_passes(codecs):
    """Header bytes overwritten in R2 and R3 and the wire cut short inside R3:
    with R0 and R1 in front these frames and tiles belong to their blocks'
    second and later passes.  Status, bytes and records equal the oracle's."""
    wire, fs, regions, _ = _wire(ORDERS[0])
    rng = np.random.default_rng(31)
    bad = np.array(wire)
    fs = np.array(fs)
    grid = _cus()
    hit = []
    for name, count in (("R2", 3), ("R3", 4)):
        lo, hi = regions[name]
        first, last = np.searchsorted(fs, lo), np.searchsorted(fs, hi)
        for i in rng.integers(first, last, count):
            # the length byte: an extended length or a payload running into the next frames
            bad[int(fs[i]) + 1] = rng.choice([0x7E, 0x7F, 0xFE, 0xFF, 0x7D])
            hit.append(int(i))
    cut = regions["R3"][0] + (regions["R3"][1] - regions["R3"][0]) * 2 // 3 + 5
    bad = bad[:cut]
    tiles = -(-len(bad) // TILE)
    assert tiles > 3 * grid and len(fs) > grid * BLOCK
    assert min(hit) >= grid * BLOCK and regions["R2"][0] // TILE >= grid   # damaged frames and tiles: later passes
    assert int(np.searchsorted(fs, cut)) < len(fs) - 1000                  # many frames past the cut
    ref = oracle.decode_batch(bad, fs)
    assert ref[0] != 0 and int((ref[2]["error"] != 0).sum()) > 1000
    c = codecs(1)
    for inplace in (False, True):
        _check(*_decode(c, bad, fs, inplace), ref)
    assert c.sync_status() == 0   # the latch is cleared


def test_decode_default_grid_control(codecs):
    """The knob unset: the grid covers every tile and every slice of frames
    (the default cap is far above both), and the bytes are the same."""
    wire, fs, _, ref = _wire(ORDERS[0])
    tiles = -(-len(wire) // TILE)
    assert _grid(tiles, len(fs), DEC_BLOCKS_PER_CU) >= tiles   # no block takes a second tile
    _check(*_decode(codecs(None), wire, fs, False), ref)


# ------------------------------------------- piece-path encode scan, 3 passes
def test_encode_piece_scan_three_passes(codecs):
    """n = 2 x 262 144 + 1 500 ragged frames (payloads 0-40 B; opcodes, masks,
    statuses and misaligned sources mixed) with a capacity past n * SMALL_AVG:
    the piece kernel, whose scan of the 514 scan-block sums (frame bytes and
    piece counts) runs its carry loop three times.  Offsets and wire against
    the oracle; the same frames through the small-frame kernel (exact
    capacity) give the same bytes."""
    n = 2 * 262144 + 1500
    assert -(-n // SCAN_ITEMS) > 2 * BLOCK   # scan-block sums: more than two passes of one block
    rng = np.random.default_rng(41)
    payload, desc = _mixed_desc(rng, n, 0, 40)
    wire_o, off_o = oracle.encode_batch(payload, desc)
    exact = int(off_o[n])
    c = codecs(None)
    p, d = dev(payload), ca.desc_to_tensor(desc, "cuda")
    for cap in (n * SMALL_AVG + 4096, exact):
        assert (cap > n * SMALL_AVG) == (cap != exact)   # the piece kernel, then the small-frame kernel
        wire, off = c.encode_batch(p, d, wire_cap=cap)
        assert c.sync_status() == 0
        assert np.array_equal(off.cpu().numpy().view(np.uint64), off_o), cap
        assert np.array_equal(wire[:exact].cpu().numpy(), wire_o), cap
        del wire


# ------------------------------- staged host pipelines, slot buffers regrown
@functools.lru_cache(maxsize=None)
def _growth_batches():
    """Three batches whose segments (1 MiB) ask the slots for different
    buffers in turn: (payload, desc, oracle's wire and offsets, oracle's decode)."""
    rng = np.random.default_rng(51)
    out = []
    for lo, hi, nbytes in ((1010, 1018, 5 << 19),       # ~2.5 MiB of ~1 KiB frames
                           (65000, 65528, 5 << 20),     # more bytes, fewer frames per segment
                           (8, 14, 3 << 19)):           # ~1.5 MiB of ~20-byte frames: more frames, fewer bytes
        lens = rng.integers(lo, hi + 1, nbytes // ((lo + hi) // 2 + 6))
        desc, total = wl.ragged_desc(rng, lens)
        desc["mask"] = rng.random(len(desc)) < 0.8
        payload = wl.random_bytes(rng, total)
        wire, off = oracle.encode_batch(payload, desc)
        out.append((payload, desc, wire, off, oracle.decode_batch(wire, off[:-1].copy())))
    return out


def test_host_pipeline_slot_buffers_regrow(monkeypatch):
    """One context ($WSG_STAGE_MB=1, pageable buffers): three staged decodes,
    then three staged encodes, each asking the slots for larger byte buffers
    and smaller frame tables than the call before it, or the reverse, so every
    slot array is freed and regrown between calls; the context destroyed at
    the end.  Every call's bytes, records and offsets equal the oracle's."""
    batches = _growth_batches()
    per_seg = [(len(w) / -(-len(w) // (1 << 20)), len(d) / -(-len(w) // (1 << 20))) for _, d, w, _, _ in batches]
    assert per_seg[1][0] >= per_seg[0][0] and per_seg[1][1] < per_seg[0][1]   # more bytes, fewer frames
    assert per_seg[2][1] > 4 * per_seg[0][1]                                  # more frames than any before
    monkeypatch.setenv("WSG_STAGE_MB", "1")   # (read at wsg_create; put back after the test)
    c = ca.Codec(0)
    try:
        for payload, desc, wire, off, ref in batches:
            assert len(wire) > (1 << 20) and ref[0] == 0   # the staged pipeline, more than one segment
            out = np.full(len(wire) + PAD, SENTINEL, dtype=np.uint8)
            rc, got, info = c.decode_batch_host(np.array(wire), off[:-1].copy(), out=out)
            _check(rc, got, info, ref)
            assert (out[len(wire):] == SENTINEL).all()
        for payload, desc, wire, off, _ in batches:
            buf = np.full(len(wire) + PAD, SENTINEL, dtype=np.uint8)
            rc, got, got_off = c.encode_batch_host(payload, desc, wire=buf)
            assert rc == 0
            assert np.array_equal(got_off, off)
            assert np.array_equal(got, wire)
            assert (buf[len(wire):] == SENTINEL).all()
    finally:
        c.close()
