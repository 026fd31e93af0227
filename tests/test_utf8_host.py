"""csrc/wsg_utf8.h under AddressSanitizer and UBSan, on the host: a stand-alone
program (its own main) runs the rule over every string of length 0..4 over the
25 boundary bytes, each in a heap block of exactly its length, so a read past
either end of a string is a report.  The expected values are Python's
decoder's, handed over in a file in the order the program enumerates.  The
program then holds the header's word-wise form of the rule (utf8_words_bad,
the kernel's filter) against the position-local one, position by position."""
import os
import shutil
import subprocess

import pytest

from tests import utf8_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wsg_utf8.h"

// usage: prog <alphabet hex> <max_len> <file of expected values, one byte per string>
// The strings in the order of length, then as numbers in base |alphabet|,
// most significant digit first.
int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    std::vector<uint8_t> alphabet;
    for (const char* p = argv[1]; p[0] && p[1]; p += 2) {
        unsigned v = 0;
        if (std::sscanf(p, "%2x", &v) != 1)
            return 2;
        alphabet.push_back(uint8_t(v));
    }
    const int max_len = std::atoi(argv[2]);
    std::FILE* f = std::fopen(argv[3], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> want;
    for (int ch; (ch = std::fgetc(f)) != EOF;)
        want.push_back(uint8_t(ch));
    std::fclose(f);
    size_t at = 0, wrong = 0;
    const size_t base = alphabet.size();
    for (int n = 0; n <= max_len; ++n) {
        size_t count = 1;
        for (int k = 0; k < n; ++k)
            count *= base;
        for (size_t v = 0; v < count; ++v, ++at) {
            uint8_t* s = static_cast<uint8_t*>(std::malloc(size_t(n)));   // exactly n bytes
            size_t digits = v;
            for (int k = n - 1; k >= 0; --k, digits /= base)
                s[k] = alphabet[digits % base];
            const uint64_t got = wsg::utf8_valid_up_to(s, uint64_t(n));
            if (at >= want.size() || got != want[at]) {
                if (wrong++ < 10) {
                    std::fprintf(stderr, "string %zu (length %d):", at, n);
                    for (int k = 0; k < n; ++k)
                        std::fprintf(stderr, " %02x", s[k]);
                    std::fprintf(stderr, " -> %llu, want %d\n", (unsigned long long)got,
                                 at < want.size() ? int(want[at]) : -1);
                }
            }
            std::free(s);
        }
    }
    if (at != want.size())
        return 3;
    std::printf("%zu strings, %zu wrong\n", at, wrong);

    // The word-wise form against the position-local one: windows of 24 bytes
    // (positions -4..19), the 16 positions 0..15 asked of both.  Every string
    // of length 0..3 at every offset of a window of zeros, every string of
    // length 4 at the four phases of a word, and random windows.
    size_t windows = 0, differ = 0;
    uint8_t win[24];
    auto compare = [&]() {
        uint32_t d[6], bad[4];
        std::memcpy(d, win, 24);   // (a little-endian host, as the device)
        wsg::utf8_words_bad(d, bad);
        auto in_window = [&](int64_t j) -> uint32_t { return j < -4 || j >= 20 ? 0u : win[j + 4]; };
        for (int i = 0; i < 16; ++i) {
            const bool a = ((bad[i >> 2] >> (8 * (i & 3))) & 0x80u) != 0;
            const bool b = wsg::utf8_bad_at(in_window, int64_t(i));
            if (((bad[i >> 2] >> (8 * (i & 3))) & 0x7Fu) != 0 || a != b) {
                if (differ++ < 10) {
                    std::fprintf(stderr, "window");
                    for (int k = 0; k < 24; ++k)
                        std::fprintf(stderr, " %02x", win[k]);
                    std::fprintf(stderr, ": position %d word-wise %d, rule %d\n", i, int(a), int(b));
                }
            }
        }
        ++windows;
    };
    for (int n = 0; n <= max_len; ++n) {
        size_t count = 1;
        for (int k = 0; k < n; ++k)
            count *= base;
        for (size_t v = 0; v < count; ++v)
            for (int off = 0; off + n <= 24 && off < (n < 4 ? 24 : 8); ++off) {
                std::memset(win, 0, sizeof win);
                size_t digits = v;
                for (int k = n - 1; k >= 0; --k, digits /= base)
                    win[off + k] = alphabet[digits % base];
                compare();
            }
    }
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (int r = 0; r < 1000000; ++r) {
        for (int k = 0; k < 24; ++k) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t pick = uint32_t(state >> 33);
            win[k] = (r & 1) ? alphabet[pick % base] : uint8_t(pick >> 8);   // boundary bytes, or any byte
        }
        compare();
    }
    std::printf("%zu windows, %zu differ\n", windows, differ);
    return wrong || differ ? 1 : 0;
}
"""


def _compile(tmp, name, text, extra=()):
    src = os.path.join(tmp, name + ".cpp")
    with open(src, "w") as f:
        f.write(text)
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *SAN, *extra, "-o", exe, src], capture_output=True, text=True)
    return exe, r


def test_rule_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = str(tmp_path)
    exe, r = _compile(tmp, "probe", "int main() { return 0; }\n")
    if r.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtime: " + r.stderr[-300:])
    exe, r = _compile(tmp, "utf8_rule", PROGRAM,
                      ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cppserver_amd", "csrc")])
    assert r.returncode == 0, r.stderr[-3000:]
    expected = os.path.join(tmp, "expected.bin")
    with open(expected, "wb") as f:
        f.write(bytes(uc.want(b) for b in uc.exhaustive(4)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, uc.BOUNDARY.hex(), "4", expected], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    lines = run.stdout.strip().splitlines()
    assert lines[0] == "%d strings, 0 wrong" % sum(25 ** k for k in range(5))
    assert lines[1].endswith(" windows, 0 differ") and int(lines[1].split()[0]) > 4000000
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
