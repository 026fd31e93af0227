"""wsg_proto_judge under AddressSanitizer + UndefinedBehaviorSanitizer (CPU
only): tests/cpp/test_proto_host.cpp, a program of its own built by
tests/cpp/proto_host.mk with the host source of the rule instrumented, run as a
program.  Every combination of opcode, fin, masked, RSV, length, open and role
against a second statement of the rule table; each call's wire is a heap block
exactly as long as the frame."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_proto_judge_sanitized():
    target = os.path.join("_build", "san", "test_proto_host")
    r = subprocess.run(["make", "-s", "-C", CPP, "-f", "proto_host.mk"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(CPP, target)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "calls ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
