// bench_upgrade_client.cpp — the client's half of the upgrade on one host core,
// measurement only (tools/upgradeclientbench.py runs it): every response of a
// case file (u32 count, then per case the 16 nonce bytes, u32 length and the
// bytes) judged by wsg_upgrade_client_judge, and fed to a fresh WSClient over
// an in-memory transport with that nonce, the way a connection reaches the C++
// classes today (HTTPResponse::Parse, PerformClientUpgrade with OpenSSL's
// SHA-1).  The cases hold the response alone: the frames behind it would go to
// the frame reader, which is not what is measured.  Both loops run `reps`
// times over the whole file; one line per repetition: "judge <ns per
// response>" / "classes <ns per response>", and at the end the accepted count
// of each (they must agree).
//   bench_upgrade_client <case file> <reps>
#include "server/ws/ws_client.h"

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
    size_t Send(const void*, size_t n) override { return n; }
    bool SendAsync(const void* b, size_t n) override { return Send(b, n) == n; }
    size_t Receive(void*, size_t) override { return 0; }
    bool Disconnect() override { return true; }
    bool IsConnected() const override { return true; }
};

struct Client : WSClient {
    using WSClient::WSClient;
    void nonce(const uint8_t* n) { std::memcpy(_ws_nonce.data(), n, 16); }
    bool handshaked() const { return _ws_handshaked; }
};

struct Case {
    const uint8_t* nonce;
    const uint8_t* data;
    uint32_t len;
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
    std::vector<Case> cases;
    size_t at = 4;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len;
        std::memcpy(&len, in.data() + at + 16, 4);
        const uint8_t* p = reinterpret_cast<const uint8_t*>(in.data()) + at;
        cases.push_back(Case{p, p + 20, len});
        at += 20 + len;
    }
    size_t judge_ok = 0, class_ok = 0;
    for (int r = 0; r < reps; ++r) {
        judge_ok = 0;
        double t0 = now_ns();
        for (const Case& q : cases) {
            wsg_upgrade_reply up;
            uint64_t consumed, need;
            if (wsg_upgrade_client_judge(q.data, q.len, q.nonce, 0, &up, &consumed, &need) != WSG_OK)
                return 1;
            judge_ok += up.code == WSG_UC_ACCEPTED;
        }
        std::printf("judge %.1f\n", (now_ns() - t0) / count);
        class_ok = 0;
        t0 = now_ns();
        for (const Case& q : cases) {
            Sink sink;
            Client client(sink);
            client.nonce(q.nonce);
            client.onReceived(q.data, q.len);
            class_ok += client.handshaked();
        }
        std::printf("classes %.1f\n", (now_ns() - t0) / count);
    }
    std::printf("accepted %zu %zu\n", judge_ok, class_ok);
    return judge_ok == class_ok ? 0 : 1;
}
