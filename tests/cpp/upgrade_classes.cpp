// upgrade_classes.cpp — what the C++ classes do to a connection's first bytes:
// each case of a case file is fed whole to a fresh WSSession over the
// in-memory transport of test_handshake.cpp, and the program reports the
// upgrade response sent, the handshaked flag and the bytes handed on as frames
// (the messages delivered and the frame reader's partial tail).  Host only:
// tests/test_upgrade_model.py compares the model with this, case by case.
//   upgrade_classes <case file> <result file>
// case file: u32 count, then per case u32 length and the bytes.
// result file: per case u8 handshaked, then three u32-length-prefixed byte
// strings: the response, the messages (opcode byte, u32 length, payload each)
// and the partial frame buffered.
#include "server/ws/ws_session.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

using namespace CppServer;
using namespace CppServer::WS;

// Host only, as in test_handshake.cpp: the receive batch's page-locked buffers
// come from wsg_host_alloc (HIP); these definitions take the place of
// libwsg.so's with heap memory, which is all a batch of key-0 frames needs.
extern "C" int wsg_host_alloc(size_t bytes, void** out)
{
    *out = std::malloc(bytes ? bytes : 1);
    return *out ? WSG_OK : WSG_ENOMEM;
}
extern "C" int wsg_host_free(void* p)
{
    std::free(p);
    return WSG_OK;
}

namespace {

struct Loop : Transport {
    std::string sent;
    size_t Send(const void* b, size_t n) override
    {
        sent.append(static_cast<const char*>(b), n);
        return n;
    }
    bool SendAsync(const void* b, size_t n) override { return Send(b, n) == n; }
    size_t Receive(void*, size_t) override { return 0; }
    bool Disconnect() override { return true; }
    bool IsConnected() const override { return true; }
};

void put_u32(std::string& out, size_t v)
{
    const uint32_t x = uint32_t(v);
    out.append(reinterpret_cast<const char*>(&x), 4);
}

struct Session : WSSession {
    using WSSession::WSSession;
    std::string response, messages;
    void SendResponse(const HTTP::HTTPResponse& r) override
    {
        response += r.cache();
        WSSession::SendResponse(r);
    }
    void message(uint8_t opcode, const void* buffer, size_t size)
    {
        messages.push_back(char(opcode));
        put_u32(messages, size);
        messages.append(static_cast<const char*>(buffer), size);
    }
    void onWSReceived(const void* buffer, size_t size) override { message(_ws_opcode, buffer, size); }
    void onWSPing(const void* buffer, size_t size) override { message(WS_PING, buffer, size); }
    void onWSPong(const void* buffer, size_t size) override { message(WS_PONG, buffer, size); }
    void onWSClose(const void* buffer, size_t size, int) override { message(WS_CLOSE, buffer, size); }
    bool handshaked() const { return _ws_handshaked; }
    std::string partial() const
    {
        if (_ws_frame_received)
            return std::string();
        return std::string(_ws_receive_frame_buffer.begin(), _ws_receive_frame_buffer.end());
    }
};

bool read_all(const char* path, std::string& out)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f)
        return false;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0)
        out.append(buf, n);
    std::fclose(f);
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    std::string in, out;
    if (argc != 3 || !read_all(argv[1], in) || in.size() < 4) {
        std::fprintf(stderr, "usage: upgrade_classes <case file> <result file>\n");
        return 2;
    }
    uint32_t count;
    std::memcpy(&count, in.data(), 4);
    size_t at = 4;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len;
        if (at + 4 > in.size())
            return 2;
        std::memcpy(&len, in.data() + at, 4);
        at += 4;
        if (at + len > in.size())
            return 2;
        Loop loop;
        Session session(loop);
        session.Connect();
        try {
            session.onReceived(in.data() + at, len);
        } catch (const std::exception&) {
            // a frame behind the request that needs the device: the upgrade is decided by then
        }
        at += len;
        out.push_back(session.handshaked() ? 1 : 0);
        put_u32(out, session.response.size());
        out += session.response;
        put_u32(out, session.messages.size());
        out += session.messages;
        const std::string partial = session.partial();
        put_u32(out, partial.size());
        out += partial;
    }
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0)
        return 2;
    return 0;
}
