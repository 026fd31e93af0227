// test_upgrade_client_host.cpp — wsg_upgrade_client_judge and
// wsg_upgrade_request (the rule wsg_upgrade_client_streams' and
// wsg_upgrade_requests' kernels run) as a program of its own, built with
// AddressSanitizer and UndefinedBehaviorSanitizer by upgrade_client.mk.  Every
// response is judged in a heap block of exactly its size, the nonce in one of
// 16 bytes, every request built into a block of exactly tpl_len bytes, so a
// read or write one byte out of place is reported.
//   test_upgrade_client_host <seed> <iterations>       the randomised driver
//   test_upgrade_client_host --cases <file> <result>   judge a case file (format
//                                                      of upgrade_client_classes.cpp);
//                                                      per case the 32-byte record,
//                                                      consumed, need (u64 each)
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
    wsg_upgrade_reply up;
    uint64_t consumed, need;
};

static Judged judge(const std::string& resp, const uint8_t* nonce16, uint64_t max_response)
{
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(resp.size() ? resp.size() : 1));
    std::memcpy(buf, resp.data(), resp.size());
    uint8_t* nonce = static_cast<uint8_t*>(std::malloc(16));
    std::memcpy(nonce, nonce16, 16);
    Judged j{};
    std::memset(&j.up, 0xA5, sizeof(j.up));
    CHECK(wsg_upgrade_client_judge(buf, resp.size(), nonce, max_response, &j.up, &j.consumed, &j.need) == WSG_OK);
    wsg_upgrade_reply again;
    CHECK(wsg_upgrade_client_judge(buf, resp.size(), nonce, max_response, &again, nullptr, nullptr) == WSG_OK);
    CHECK(std::memcmp(&again, &j.up, sizeof(again)) == 0);
    // what holds for every outcome
    CHECK(j.up._pad == 0 && j.up._zero == 0 && j.up.code <= WSG_UC_TOO_LONG);
    CHECK(j.consumed <= resp.size());
    CHECK(uint64_t(j.up.accept_off) + j.up.accept_len <= resp.size());
    const bool unfinished = j.up.code == WSG_UC_INCOMPLETE || j.up.code == WSG_UC_TOO_LONG;
    if (unfinished)
        CHECK(j.consumed == 0 && j.up.status == 0 && (j.need == 0 || j.need > resp.size()));
    else
        CHECK(j.need == 0 && j.consumed >= 4);
    if (unfinished || j.up.code == WSG_UC_BAD_HTTP)
        CHECK(j.up.status == 0 && j.up.body_off == 0 && j.up.body_len == 0 && j.up.accept_off == 0);
    else
        CHECK(j.up.status <= 999 && j.up.body_off + j.up.body_len == j.consumed);
    CHECK((j.up.code == WSG_UC_NOT_101) == (!unfinished && j.up.code != WSG_UC_BAD_HTTP && j.up.status != 101));
    if (j.up.code == WSG_UC_NOT_101)
        CHECK(j.up.accept_off == 0 && j.up.accept_len == 0);
    if (j.up.code == WSG_UC_BAD_ACCEPT || j.up.code == WSG_UC_ACCEPTED)
        CHECK(j.up.accept_off != 0);
    std::free(nonce);
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
    static const char inserts[] = {' ', '\t', '\r', '\n', ':', ',', '\0', char(0xFF), '=', '-', 'A', '1'};
    const int edits = 1 + int(next() % 4);
    for (int e = 0; e < edits; ++e) {
        const size_t at = s.empty() ? 0 : next() % s.size();
        switch (next() % 7) {
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
        case 5:   // inside the status line and the accept value
            if (s.size() > 120)
                s[next() % 2 ? 9 + next() % 4 : 97 + next() % 28] = inserts[next() % sizeof(inserts)];
            break;
        default:
            if (next() % 4 == 0)
                s.erase(at);
            break;
        }
    }
    return s;
}

static void requests()
{
    static const char abc[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    for (uint32_t tpl_len = 24; tpl_len < 90; ++tpl_len)
        for (uint32_t key_at = 0; key_at + 24 <= tpl_len; key_at += 1 + next() % 7) {
            uint8_t* tpl = static_cast<uint8_t*>(std::malloc(tpl_len));
            uint8_t* out = static_cast<uint8_t*>(std::malloc(tpl_len));
            uint8_t* nonce = static_cast<uint8_t*>(std::malloc(16));
            for (uint32_t i = 0; i < tpl_len; ++i)
                tpl[i] = uint8_t(next());
            for (uint32_t i = 0; i < 16; ++i)
                nonce[i] = uint8_t(next());
            CHECK(wsg_upgrade_request(tpl, tpl_len, key_at, nonce, out) == WSG_OK);
            // Base64 of the nonce, worked out here
            char key[24];
            for (int g = 0; g < 6; ++g) {
                const uint32_t v = uint32_t(nonce[3 * g]) << 16 | (g < 5 ? uint32_t(nonce[3 * g + 1]) << 8 | nonce[3 * g + 2] : 0u);
                key[4 * g] = abc[v >> 18];
                key[4 * g + 1] = abc[(v >> 12) & 63];
                key[4 * g + 2] = g < 5 ? abc[(v >> 6) & 63] : '=';
                key[4 * g + 3] = g < 5 ? abc[v & 63] : '=';
            }
            CHECK(std::memcmp(out, tpl, key_at) == 0 && std::memcmp(out + key_at, key, 24) == 0 &&
                  std::memcmp(out + key_at + 24, tpl + key_at + 24, tpl_len - key_at - 24) == 0);
            CHECK(wsg_upgrade_request(tpl, tpl_len, tpl_len - 23, nonce, out) == WSG_EINVAL);
            CHECK(wsg_upgrade_request(nullptr, tpl_len, key_at, nonce, out) == WSG_EINVAL);
            std::free(nonce);
            std::free(out);
            std::free(tpl);
        }
    uint8_t b[24] = {};
    CHECK(wsg_upgrade_request(b, 23, 0, b, b) == WSG_EINVAL && wsg_upgrade_request(b, 0, 0, b, b) == WSG_EINVAL);
    CHECK(wsg_upgrade_request(b, 24, 0xFFFFFFF0u, b, b) == WSG_EINVAL);
}

static int run_random(uint64_t seed, long iterations)
{
    g_rng = seed * 0x9E3779B97F4A7C15ull + 1;
    const uint8_t* nonce = reinterpret_cast<const uint8_t*>("the sample nonce");
    const std::string base =
        "HTTP/1.1 101 Switching Protocols\r\nConnection: Upgrade\r\nUpgrade: websocket\r\n"
        "Sec-WebSocket-Accept: s3pPLMBiTxaQ9kYGzzhZRbK+xOo=\r\nContent-Length: 3\r\n\r\nabc\x81\x02hi";
    // the known answer (RFC 6455 1.3) before anything random
    const Judged k = judge(base, nonce, 0);
    CHECK(k.up.code == WSG_UC_ACCEPTED && k.consumed == base.size() - 4 && k.up.status == 101 && k.up.accept_off == 97 &&
          k.up.accept_len == 28 && k.up.body_len == 3);
    uint8_t other[16] = {};
    CHECK(judge(base, other, 0).up.code == WSG_UC_BAD_ACCEPT);
    wsg_upgrade_reply r;
    CHECK(wsg_upgrade_client_judge(nullptr, 4, nonce, 0, &r, nullptr, nullptr) == WSG_EINVAL);
    CHECK(wsg_upgrade_client_judge(nonce, 4, nullptr, 0, &r, nullptr, nullptr) == WSG_EINVAL);
    CHECK(wsg_upgrade_client_judge(nonce, 4, nonce, 0, nullptr, nullptr, nullptr) == WSG_EINVAL);
    CHECK(wsg_upgrade_client_judge(nullptr, 0, nonce, 0, &r, nullptr, nullptr) == WSG_OK && r.code == WSG_UC_INCOMPLETE);
    requests();
    long counts[WSG_UC_TOO_LONG + 1] = {};
    for (long i = 0; i < iterations; ++i) {
        const std::string resp = mutate(base);
        const uint64_t max_response = next() % 3 ? 0 : next() % (resp.size() + 2);
        uint8_t n2[16];
        for (int b = 0; b < 16; ++b)
            n2[b] = uint8_t(next());
        ++counts[judge(resp, next() % 8 ? nonce : n2, max_response).up.code];
    }
    for (int c = 0; c <= WSG_UC_TOO_LONG; ++c)
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
        if (at + 20 > in.size())
            return 2;
        const uint8_t* nonce = reinterpret_cast<const uint8_t*>(in.data() + at);
        std::memcpy(&len, in.data() + at + 16, 4);
        at += 20;
        if (at + len > in.size())
            return 2;
        const Judged j = judge(in.substr(at, len), nonce, 0);
        at += len;
        out.append(reinterpret_cast<const char*>(&j.up), sizeof(j.up));
        out.append(reinterpret_cast<const char*>(&j.consumed), 8);
        out.append(reinterpret_cast<const char*>(&j.need), 8);
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
    std::fprintf(stderr, "usage: test_upgrade_client_host <seed> <iterations> | --cases <file> <result>\n");
    return 2;
}
