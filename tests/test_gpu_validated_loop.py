"""The validating echo server's loop as one call per round, on the GPU.

tests/server_loop_cases.py's driver over the schedules and configurations of
tests/test_gpu_server_loop.py's validating form, but a round is one
wsg_reply_validated_streams and one wsg_sync: no frame table, message buffer
or verdict array passes through the host's hands.  Every connection's output
must be what checked_reply_cases.expected builds for the whole connection in
one call, its verdict the one an outside RFC 6455 reader recorded in
tests/golden/rfc6455.json, and the runs must agree with the model's step."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import server_loop_cases as sl  # noqa: E402
from tests import test_gpu_server_loop as gl  # noqa: E402
from tests.test_gpu_protocol import BLOCK  # noqa: E402
from tests.test_rfc6455_model import CONFIGS, check_schedules  # noqa: E402

VALIDATING = [c for c in CONFIGS if c.values[1]]   # the configurations with UTF-8 validation


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def one_call_step(codec, rule, mask, limit):
    """One wsg_reply_validated_streams and one wsg_sync."""
    def step(wire, spans, opcodes, proto, keys, frame_cap):
        rd = gl.Round(wire, spans, opcodes, proto, keys, frame_cap)
        o = rd.o
        valid = gl.sent((frame_cap + gl.EXTRA) * 8).view(torch.int64)
        utf8_result = gl.sent((4 + gl.EXTRA) * 8).view(torch.int64)
        out = codec.reply_validated_streams(rd.wire, rd.spans, proto=o.proto, role=pc.SERVER, max_message=limit,
                                            which=sl.WHICH, reply_op=rule, mask=mask, send_keys=rd.keys,
                                            state=o.state, frame_start=rd.fs, frame_cap=frame_cap, stream_first=rd.sf,
                                            reply=o.reply, reply_cap=rd.cap, reply_off=o.reply_off,
                                            stream_reply=o.stream_reply, close_off=o.close_off, verdict=o.verdict,
                                            result=o.result, valid=valid, utf8_result=utf8_result, msgs=o.msgs,
                                            count=o.count, info=o.info)
        assert codec.sync_status() == 0
        r = rd.finish(out[-1], lowered_on_device=True)
        nm = int(o.count[0].item())
        v = valid.cpu().numpy().view(np.uint64)
        u = utf8_result.cpu().numpy().view(np.uint64)
        assert (v[nm:] == gl.SENT64).all() and (u[4:] == gl.SENT64).all()
        lens = o.msgs.cpu().numpy().view(layout.MSG)["len"][:nm]
        assert int(u[0]) == int((v[:nm] < lens).sum())      # d_utf8_result counts what d_valid shows
        return r
    return step


def test_there_are_validating_configs():
    assert len(VALIDATING) == 2


@pytest.mark.parametrize("limit,validating,rule,mask", VALIDATING)
def test_loop(codec, limit, validating, rule, mask):
    """Three schedules of cut reads: every connection's output is the one
    call's over the whole connection, its verdict the recorded reader's, the
    three runs are identical, and some connection fails for its text."""
    keys = sl.send_keys() if mask else None
    step = one_call_step(codec, rule, mask, limit)
    runs = [sl.drive(step, seed, keys) for seed in gl.SCHEDULES]
    for seed, run in zip(gl.SCHEDULES, runs):
        sl.check_run(run, limit, validating, rule, mask, "schedule %d" % seed)
    for run in runs[1:]:
        assert run.out == runs[0].out and run.verdict == runs[0].verdict
    check_schedules(runs)
    assert all(r.max_streams > BLOCK and r.max_frames > BLOCK for r in runs)
    closed = sum(1 for v in runs[0].verdict if v != sl.NONE)
    assert closed >= 50 and any(v[0] == layout.PV_UTF8 for v in runs[0].verdict)


def test_against_the_model_step(codec):
    """One schedule driven by the model's step (tests/server_loop_cases.py::
    model_step, validating) gives the same outputs and verdicts as the device's."""
    limit, validating, rule, mask = VALIDATING[0].values
    keys = sl.send_keys() if mask else None
    dev_run = sl.drive(one_call_step(codec, rule, mask, limit), gl.SCHEDULES[0], keys)
    cpu_run = sl.drive(sl.model_step(rule, mask, limit, True), gl.SCHEDULES[0], keys)
    assert dev_run.out == cpu_run.out and dev_run.verdict == cpu_run.verdict
    sl.check_against_reader(dev_run.verdict, limit, True, "one call per round")
