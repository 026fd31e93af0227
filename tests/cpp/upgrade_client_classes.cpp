// upgrade_client_classes.cpp — what the C++ classes do to a client
// connection's first bytes: each case of a case file is fed whole to a fresh
// WSClient over an in-memory transport, its nonce set from the case, and the
// program reports the handshaked flag, the onWSError text and the bytes handed
// on as frames (the messages delivered and the frame reader's partial tail).
// Host only: tests/test_upgrade_client_model.py compares the model with this,
// case by case.
//   upgrade_client_classes <case file> <result file>
//   upgrade_client_classes --request <result file>
// case file: u32 count, then per case the 16 nonce bytes, u32 length and the
// bytes.  result file: per case u8 handshaked, then three u32-length-prefixed
// byte strings: the error text, the messages (opcode byte, u32 length, payload
// each) and the partial frame buffered.
// --request: the bytes Connect() sends for the reference test's header set
// with the nonce "the sample nonce" (HTTPRequest's serialisation).
#include "server/ws/ws_client.h"
#include "server/ws/ws_handshake.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

using namespace CppServer;
using namespace CppServer::WS;

// Host only, as in upgrade_classes.cpp: heap memory in the place of the
// page-locked buffers of wsg_host_alloc, which is all a batch of unmasked
// frames needs.
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

struct Client : WSClient {
    using WSClient::WSClient;
    std::string error, messages;
    void nonce(const char* n) { std::memcpy(_ws_nonce.data(), n, 16); }
    void onWSConnecting(HTTP::HTTPRequest& request) override
    {
        request.SetBegin("GET", "/");
        request.SetHeader("Host", "localhost");
        request.SetHeader("Origin", "http://localhost");
        request.SetHeader("Upgrade", "websocket");
        request.SetHeader("Connection", "Upgrade");
        request.SetHeader("Sec-WebSocket-Key", Base64Encode(ws_nonce()));
        request.SetHeader("Sec-WebSocket-Protocol", "chat, superchat");
        request.SetHeader("Sec-WebSocket-Version", "13");
    }
    void onWSError(const std::string& message) override { error += message; }
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

bool write_all(const char* path, const std::string& out)
{
    std::FILE* f = std::fopen(path, "wb");
    return f && std::fwrite(out.data(), 1, out.size(), f) == out.size() && std::fclose(f) == 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && std::strcmp(argv[1], "--request") == 0) {
        Loop loop;
        Client client(loop);
        client.nonce("the sample nonce");
        client.Connect();
        return write_all(argv[2], loop.sent) ? 0 : 2;
    }
    std::string in, out;
    if (argc != 3 || !read_all(argv[1], in) || in.size() < 4) {
        std::fprintf(stderr, "usage: upgrade_client_classes <case file> <result file> | --request <result file>\n");
        return 2;
    }
    uint32_t count;
    std::memcpy(&count, in.data(), 4);
    size_t at = 4;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len;
        if (at + 20 > in.size())
            return 2;
        const char* nonce = in.data() + at;
        std::memcpy(&len, in.data() + at + 16, 4);
        at += 20;
        if (at + len > in.size())
            return 2;
        Loop loop;
        Client client(loop);
        client.nonce(nonce);
        client.Connect();
        try {
            client.onReceived(in.data() + at, len);
        } catch (const std::exception&) {
            // a frame behind the response that needs the device: the upgrade is decided by then
        }
        at += len;
        out.push_back(client.handshaked() ? 1 : 0);
        put_u32(out, client.error.size());
        out += client.error;
        put_u32(out, client.messages.size());
        out += client.messages;
        const std::string partial = client.partial();
        put_u32(out, partial.size());
        out += partial;
    }
    return write_all(argv[2], out) ? 0 : 2;
}
