// test_upgrade_host.cpp — wsg_upgrade_judge (the rule wsg_upgrade_streams'
// kernels run) as a program of its own, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by upgrade_host.mk.  Every request is judged in
// a heap block of exactly its size, the response written to one of exactly
// resp_len bytes, so a read or write one byte out of place is reported.
//   test_upgrade_host <seed> <iterations>       the randomised driver
//   test_upgrade_host --cases <file> <result>   judge a case file (format of
//                                               upgrade_classes.cpp); per case
//                                               the 32-byte record, consumed,
//                                               need (u64 each), the response
#include "wsg_capi.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            ++g_failures;                                                              \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                              \
    } while (0)

struct Judged {
    wsg_upgrade up;
    uint64_t consumed, need;
    std::string resp;
};

static Judged judge(const std::string& req, uint64_t max_request)
{
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(req.size() ? req.size() : 1));
    std::memcpy(buf, req.data(), req.size());
    Judged j{};
    // the sizes first, then the response into a block of exactly that size
    CHECK(wsg_upgrade_judge(buf, req.size(), max_request, &j.up, nullptr, 0, &j.consumed, &j.need) ==
          (j.up.resp_len ? WSG_ENOMEM : WSG_OK));
    uint8_t* resp = static_cast<uint8_t*>(std::malloc(j.up.resp_len ? j.up.resp_len : 1));
    wsg_upgrade again;
    uint64_t c2 = 0, n2 = 0;
    CHECK(wsg_upgrade_judge(buf, req.size(), max_request, &again, resp, j.up.resp_len, &c2, &n2) == WSG_OK);
    CHECK(std::memcmp(&again, &j.up, sizeof(again)) == 0 && c2 == j.consumed && n2 == j.need);
    if (j.up.resp_len)
        CHECK(wsg_upgrade_judge(buf, req.size(), max_request, &again, resp, j.up.resp_len - 1, &c2, &n2) == WSG_ENOMEM);
    j.resp.assign(reinterpret_cast<const char*>(resp), j.up.resp_len);
    // what holds for every outcome
    CHECK(j.up._pad == 0 && j.up.resp_len <= WSG_UPGRADE_RESP_MAX && j.up.code <= WSG_UP_TOO_LONG);
    CHECK(j.up.status == (j.up.code == WSG_UP_ACCEPTED ? 101 : j.up.resp_len ? 400 : 0));
    CHECK(j.consumed <= req.size());
    CHECK(uint64_t(j.up.key_off) + j.up.key_len <= req.size() && uint64_t(j.up.url_off) + j.up.url_len <= req.size());
    const bool unfinished = j.up.code == WSG_UP_INCOMPLETE || j.up.code == WSG_UP_TOO_LONG;
    if (unfinished)
        CHECK(j.consumed == 0 && j.up.resp_len == 0 && (j.need == 0 || j.need > req.size()));
    else
        CHECK(j.need == 0 && j.consumed >= 4);
    if (j.up.code == WSG_UP_ACCEPTED)
        CHECK(j.up.resp_len == 148 && j.up.key_len > 0 && j.resp.compare(0, 12, "HTTP/1.1 101") == 0);
    std::free(resp);
    std::free(buf);
    return j;
}

static uint64_t g_rng = 1;
static uint64_t next()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static std::string mutate(std::string s)
{
    static const char inserts[] = {' ', '\t', '\r', '\n', ':', ',', '\0', char(0xFF)};
    const int edits = 1 + int(next() % 4);
    for (int e = 0; e < edits; ++e) {
        const size_t at = s.empty() ? 0 : next() % s.size();
        switch (next() % 6) {
        case 0:
            if (!s.empty())
                s[at] = char(uint8_t(s[at]) ^ (1u << (next() % 8)));
            break;
        case 1:
            s.insert(at, 1, inserts[next() % sizeof(inserts)]);
            break;
        case 2:
            s.erase(at, 1 + next() % 3);
            break;
        case 3:
            s.insert(at, "\r\n");
            break;
        case 4:
            s.insert(at, s.substr(next() % (s.size() + 1), next() % 40));
            break;
        default:
            if (next() % 4 == 0)
                s.erase(at);
            break;
        }
    }
    return s;
}

static int run_random(uint64_t seed, long iterations)
{
    g_rng = seed * 0x9E3779B97F4A7C15ull + 1;
    const std::string base =
        "GET /chat HTTP/1.1\r\nHost: server.example.com\r\nUpgrade: websocket\r\nConnection: keep-alive, Upgrade\r\n"
        "Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\nContent-Length: 3\r\nSec-WebSocket-Version: 13\r\n\r\nabcdef";
    // the known answer (RFC 6455 1.3) before anything random
    const Judged k = judge(base, 0);
    CHECK(k.up.code == WSG_UP_ACCEPTED && k.consumed == base.size() - 3);
    CHECK(k.resp.find("Sec-WebSocket-Accept: s3pPLMBiTxaQ9kYGzzhZRbK+xOo=\r\n") != std::string::npos);
    long counts[WSG_UP_TOO_LONG + 1] = {};
    for (long i = 0; i < iterations; ++i) {
        const std::string req = mutate(base);
        const uint64_t max_request = next() % 3 ? 0 : next() % (req.size() + 2);
        ++counts[judge(req, max_request).up.code];
    }
    for (int c = 0; c <= WSG_UP_TOO_LONG; ++c)
        std::printf("code %d: %ld\n", c, counts[c]);
    std::printf("%d failures\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}

static int run_cases(const char* in_path, const char* out_path)
{
    std::FILE* f = std::fopen(in_path, "rb");
    if (!f)
        return 2;
    std::string in;
    char chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0)
        in.append(chunk, n);
    std::fclose(f);
    if (in.size() < 4)
        return 2;
    uint32_t count;
    std::memcpy(&count, in.data(), 4);
    size_t at = 4;
    std::string out;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len;
        if (at + 4 > in.size())
            return 2;
        std::memcpy(&len, in.data() + at, 4);
        at += 4;
        if (at + len > in.size())
            return 2;
        const Judged j = judge(in.substr(at, len), 0);
        at += len;
        out.append(reinterpret_cast<const char*>(&j.up), sizeof(j.up));
        out.append(reinterpret_cast<const char*>(&j.consumed), 8);
        out.append(reinterpret_cast<const char*>(&j.need), 8);
        out += j.resp;
    }
    f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0)
        return 2;
    std::printf("%u cases, %d failures\n", count, g_failures);
    return g_failures == 0 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::strcmp(argv[1], "--cases") == 0)
        return run_cases(argv[2], argv[3]);
    if (argc == 3)
        return run_random(std::strtoull(argv[1], nullptr, 10), std::strtol(argv[2], nullptr, 10));
    std::fprintf(stderr, "usage: test_upgrade_host <seed> <iterations> | --cases <file> <result>\n");
    return 2;
}
