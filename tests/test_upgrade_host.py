"""wsg_upgrade_judge under AddressSanitizer and UndefinedBehaviorSanitizer.

tests/cpp/test_upgrade_host.cpp is a program of its own (built by
tests/cpp/upgrade_host.mk from the rule's host source, instrumented; no
preload, no GPU): every request lies in a heap block of exactly its size and
the response goes to one of exactly its length.  It runs a randomised driver,
and judges the case file of tests/upgrade_cases.py, whose results must be the
model's."""
import os
import struct
import subprocess

import numpy as np
import pytest

from cppserver_amd import layout
from tests import upgrade_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PROGRAM = os.path.join(CPP, "_build", "san", "test_upgrade_host")


@pytest.fixture(scope="module", autouse=True)
def program():
    target = os.path.join("_build", "san", "test_upgrade_host")
    r = subprocess.run(["make", "-s", "-C", CPP, "-f", "upgrade_host.mk", target], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def run(args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([PROGRAM] + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("seed", [1, 6455])
def test_randomised_driver(seed):
    out = run([str(seed), "20000"])
    assert "0 failures" in out
    counts = dict((int(a), int(b)) for a, b in (ln[5:].split(": ") for ln in out.splitlines() if ln.startswith("code ")))
    assert sum(counts.values()) == 20000
    assert sum(1 for v in counts.values() if v) >= 8, counts   # the driver reaches the rule's branches


def test_cases_under_the_sanitizers(tmp_path):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "judged.bin")
    with open(src, "wb") as f:
        f.write(uc.pack_cases(uc.all_cases()))
    assert "0 failures" in run(["--cases", src, dst])
    with open(dst, "rb") as f:
        out = f.read()
    at = 0
    for data, e in zip(uc.all_cases(), uc.expected()):
        rec = np.frombuffer(out, dtype=layout.UPGRADE_DTYPE, count=1, offset=at)[0]
        consumed, need = struct.unpack_from("<QQ", out, at + 32)
        n = int(rec["resp_len"])
        resp = out[at + 48:at + 48 + n]
        at += 48 + n
        assert (int(rec["code"]), int(rec["status"]), resp, consumed, need) == (
            e["code"], e["status"], e["resp"], e["consumed"], e["need"]), data
        assert (int(rec["key_off"]), int(rec["key_len"])) == e["key"], data
    assert at == len(out)
