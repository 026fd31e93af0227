// The argument checks of wsg_upgrade_client_streams and wsg_upgrade_requests
// (args_upgrade_client, args_upgrade_requests of cppserver_amd/csrc/wsg_args.h)
// without a device, as test_capi_args.cpp checks the older entry points':
// every operand as a literal row — name, bytes, alignment, whether it may be
// null — written out from the contract text of wsg_capi.h.  Pointers are
// addresses inside one static buffer and are never dereferenced; in_alloc is
// this program's: it records every query and can refuse the k-th.  Built with
// AddressSanitizer + UndefinedBehaviorSanitizer by upgrade_client.mk.
#include "wsg_args.h"

#include <cstdio>
#include <utility>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, what); \
        }                                                                   \
    } while (0)

using uc = unsigned char;
std::vector<std::pair<const void*, uint64_t>> asked;
int refuse_at = -1;

alignas(64) uc arena[64 * 8];
uc* slot(size_t i) { return arena + 64 * i; }

struct Row {
    const char* name;
    uint64_t bytes;
    uint32_t align;
    bool sized;   // null allowed when bytes == 0 (else never)
};

} // namespace

bool in_alloc(const void* p, uint64_t bytes)
{
    asked.push_back({p, bytes});
    return int(asked.size()) - 1 != refuse_at;
}

namespace {

// rows: the operands in the order of `call`'s pointers; checks null, every
// misalignment below the row's, what in_alloc is asked, each refusal.
template <class Call>
void table(const char* what, const std::vector<Row>& rows, Call call)
{
    std::vector<uc*> p;
    for (size_t i = 0; i < rows.size(); ++i)
        p.push_back(slot(i));
    asked.clear();
    refuse_at = -1;
    CHECK(call(p, false) == WSG_OK && asked.empty());
    CHECK(call(p, true) == WSG_OK && asked.size() == rows.size());
    for (size_t i = 0; i < rows.size() && i < asked.size(); ++i)
        CHECK(asked[i].first == p[i] && asked[i].second == rows[i].bytes);
    for (size_t i = 0; i < rows.size(); ++i) {
        refuse_at = int(i);
        asked.clear();
        CHECK(call(p, true) == WSG_EINVAL);
        refuse_at = -1;
        std::vector<uc*> q = p;
        q[i] = nullptr;
        asked.clear();
        CHECK(call(q, true) == WSG_EINVAL && asked.empty());
        for (uint32_t d = 1; d < 16; ++d) {
            q[i] = p[i] + d;
            CHECK((call(q, false) == WSG_OK) == (d % rows[i].align == 0));
        }
    }
}

} // namespace

int main()
{
    {
        const char* what = "wsg_upgrade_client_streams";
        // three streams in a wire of 33 bytes: read to the end of its last 16-byte block
        const std::vector<Row> rows = {{"d_wire", 48, 16, true}, {"d_span", 3 * 32, 8, true}, {"d_nonce", 3 * 16, 16, true},
                                       {"d_up", 3 * 32, 8, true}, {"d_count", 3 * 8, 8, false}};
        table(what, rows, [](const std::vector<uc*>& p, bool check) {
            return wsg::args_upgrade_client(p[0], 33, p[1], 3, p[2], p[3], p[4], check);
        });
        // no stream, no byte: the count alone
        asked.clear();
        CHECK(wsg::args_upgrade_client(nullptr, 0, nullptr, 0, nullptr, nullptr, slot(4), true) == WSG_OK);
        CHECK(asked.size() == 1 && asked[0].first == slot(4) && asked[0].second == 24);
        CHECK(wsg::args_upgrade_client(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, false) == WSG_EINVAL);
        CHECK(wsg::args_upgrade_client(slot(0), 33, slot(1), UINT32_MAX, slot(2), slot(3), slot(4), false) == WSG_EINVAL);
        // empty streams over no wire
        CHECK(wsg::args_upgrade_client(nullptr, 0, slot(1), 3, slot(2), slot(3), slot(4), false) == WSG_OK);
    }
    {
        const char* what = "wsg_upgrade_requests";
        // five requests of 41 bytes: the template read to the end of its last 16-byte block
        const std::vector<Row> rows = {{"d_tpl", 48, 16, false}, {"d_nonce", 5 * 16, 16, true}, {"d_req", 5 * 41, 16, false}};
        table(what, rows, [](const std::vector<uc*>& p, bool check) {
            return wsg::args_upgrade_requests(p[0], 41, 17, p[1], 5, p[2], 5 * 41, check);
        });
        CHECK(wsg::args_upgrade_requests(slot(0), 41, 17, slot(1), 5, slot(2), 5 * 41, false) == WSG_OK);
        CHECK(wsg::args_upgrade_requests(slot(0), 41, 18, slot(1), 5, slot(2), 5 * 41, false) == WSG_EINVAL);
        CHECK(wsg::args_upgrade_requests(slot(0), 23, 0, slot(1), 5, slot(2), 5 * 23, false) == WSG_EINVAL);
        CHECK(wsg::args_upgrade_requests(slot(0), 0, 0, slot(1), 5, slot(2), 0, false) == WSG_EINVAL);
        CHECK(wsg::args_upgrade_requests(slot(0), 24, 0xFFFFFFF0u, slot(1), 5, slot(2), 5 * 24, false) == WSG_EINVAL);
        // no request: nothing needed, nothing looked up
        asked.clear();
        CHECK(wsg::args_upgrade_requests(nullptr, 41, 17, nullptr, 0, nullptr, 0, true) == WSG_OK && asked.empty());
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
