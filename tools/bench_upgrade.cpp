// bench_upgrade.cpp — the upgrade handshake on one host core, measurement only
// (tools/upgradebench.py runs it): every request of a case file (u32 count,
// then per request u32 length and the bytes) judged by wsg_upgrade_judge, and
// fed to a fresh WSSession over an in-memory transport, the way a connection
// reaches the C++ classes today.  Both loops run `reps` times over the whole
// file; one line per repetition: "judge <ns per request>" / "classes <ns per
// request>", and at the end the responses' byte count of each (they must agree).
//   bench_upgrade <case file> <reps>
#include "server/ws/ws_session.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace CppServer;
using namespace CppServer::WS;

namespace {

struct Sink : Transport {
    size_t bytes = 0;
    size_t Send(const void*, size_t n) override
    {
        bytes += n;
        return n;
    }
    bool SendAsync(const void* b, size_t n) override { return Send(b, n) == n; }
    size_t Receive(void*, size_t) override { return 0; }
    bool Disconnect() override { return true; }
    bool IsConnected() const override { return true; }
};

double now_ns()
{
    return double(std::chrono::duration_cast<std::chrono::nanoseconds>(
                      std::chrono::steady_clock::now().time_since_epoch())
                      .count());
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3)
        return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f)
        return 2;
    std::string in;
    char chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0)
        in.append(chunk, n);
    std::fclose(f);
    const int reps = std::atoi(argv[2]);
    uint32_t count;
    std::memcpy(&count, in.data(), 4);
    std::vector<std::pair<const uint8_t*, uint32_t>> req;
    size_t at = 4;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len;
        std::memcpy(&len, in.data() + at, 4);
        req.emplace_back(reinterpret_cast<const uint8_t*>(in.data()) + at + 4, len);
        at += 4 + len;
    }
    size_t judge_bytes = 0, class_bytes = 0;
    for (int r = 0; r < reps; ++r) {
        uint8_t resp[WSG_UPGRADE_RESP_MAX];
        judge_bytes = 0;
        double t0 = now_ns();
        for (const auto& q : req) {
            wsg_upgrade up;
            uint64_t consumed, need;
            if (wsg_upgrade_judge(q.first, q.second, 0, &up, resp, sizeof(resp), &consumed, &need) != WSG_OK)
                return 1;
            judge_bytes += up.resp_len;
        }
        std::printf("judge %.1f\n", (now_ns() - t0) / count);
        class_bytes = 0;
        t0 = now_ns();
        for (const auto& q : req) {
            Sink sink;
            WSSession session(sink);
            session.Connect();
            session.onReceived(q.first, q.second);
            class_bytes += sink.bytes;
        }
        std::printf("classes %.1f\n", (now_ns() - t0) / count);
    }
    std::printf("bytes %zu %zu\n", judge_bytes, class_bytes);
    return judge_bytes == class_bytes ? 0 : 1;
}
