"""wsg_upgrade_client_judge and wsg_upgrade_request under AddressSanitizer and
UndefinedBehaviorSanitizer, and the argument tables of the two device entry
points.

tests/cpp/test_upgrade_client_host.cpp is a program of its own (built by
tests/cpp/upgrade_client.mk from the rule's host source, instrumented; no
preload, no GPU): every response lies in a heap block of exactly its size, the
nonce in one of 16 bytes, every request is built into a block of exactly its
length.  It runs a randomised driver, and judges the case file of
tests/upgrade_client_cases.py, whose results must be the model's.
tests/cpp/test_upgrade_client_args.cpp checks args_upgrade_client and
args_upgrade_requests with a recording in_alloc."""
import os
import struct
import subprocess

import numpy as np
import pytest

from cppserver_amd import layout
from tests import upgrade_client_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PROGRAM = os.path.join(CPP, "_build", "san", "test_upgrade_client_host")
ARGS = os.path.join(CPP, "_build", "san", "test_upgrade_client_args")


@pytest.fixture(scope="module", autouse=True)
def programs():
    targets = [os.path.join("_build", "san", "test_upgrade_client_host"),
               os.path.join("_build", "san", "test_upgrade_client_args")]
    r = subprocess.run(["make", "-s", "-C", CPP, "-f", "upgrade_client.mk"] + targets, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def run(program, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([program] + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("seed", [1, 6455])
def test_randomised_driver(seed):
    out = run(PROGRAM, [str(seed), "20000"])
    assert "0 failures" in out
    counts = dict((int(a), int(b)) for a, b in (ln[5:].split(": ") for ln in out.splitlines() if ln.startswith("code ")))
    assert sum(counts.values()) == 20000
    assert all(counts[c] for c in range(layout.UC_TOO_LONG + 1)), counts   # the driver reaches every outcome


def test_cases_under_the_sanitizers(tmp_path):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "judged.bin")
    with open(src, "wb") as f:
        f.write(uc.pack_cases(uc.all_cases()))
    assert "0 failures" in run(PROGRAM, ["--cases", src, dst])
    with open(dst, "rb") as f:
        out = f.read()
    assert len(out) == 48 * len(uc.all_cases())
    for i, ((data, nonce), e) in enumerate(zip(uc.all_cases(), uc.expected())):
        rec = np.frombuffer(out, dtype=layout.UPGRADE_REPLY_DTYPE, count=1, offset=48 * i)[0]
        consumed, need = struct.unpack_from("<QQ", out, 48 * i + 32)
        assert (int(rec["code"]), int(rec["status"]), consumed, need) == (
            e["code"], e["status"], e["consumed"], e["need"]), data
        assert (int(rec["accept_off"]), int(rec["accept_len"])) == (e["accept"] or (0, 0)), data
        assert (int(rec["body_off"]), int(rec["body_len"])) == (e["body"] or (0, 0)), data


def test_argument_tables():
    assert "0 failures" in run(ARGS, [])
