"""Child process of tests/test_gpu_messages.py: wsg_decode_messages under
$WSG_CHECK=1 (read at wsg_create, so the context is made here).  A d_msgs
block one record short is refused with WSG_EINVAL before anything is launched;
the same call with a block of n records runs.  The blocks are exact hipMalloc
blocks (torch's allocator hands out views of larger segments).  Prints one
JSON line."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cppserver_amd as ca  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_STATE  # noqa: E402


def main():
    assert os.environ.get("WSG_CHECK") == "1"
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    vp = ctypes.c_void_p
    n = (2 << 20) // MSG.itemsize + 1       # n records end 8 bytes past 2 MiB, n - 1 end inside it
    blocks = []

    def hip_alloc(nbytes):
        p = vp()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        blocks.append(p)
        return p.value

    c = ca.Codec(0)
    res = {"ok": False}
    try:
        wire = np.tile(np.array([0x81, 0x01, 0x41], dtype=np.uint8), n)   # n unmasked text frames "A"
        d_wire = torch.from_numpy(wire).cuda()
        d_fs = torch.arange(n, dtype=torch.int64, device="cuda") * 3
        d_sf = torch.tensor([0, n], dtype=torch.int32, device="cuda")

        def call(d_msgs):
            state = torch.zeros(STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
            msg = torch.full((len(wire),), 0xA5, dtype=torch.uint8, device="cuda")
            count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
            info = torch.full((n * RECV_INFO.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = c._L.wsg_decode_messages(c._ctx, vp(d_wire.data_ptr()), len(wire), vp(d_fs.data_ptr()), n,
                                          vp(d_sf.data_ptr()), 1, vp(state.data_ptr()), vp(msg.data_ptr()), len(wire),
                                          vp(d_msgs), vp(count.data_ptr()), vp(info.data_ptr()), None)
            st = c.sync_status()
            torch.cuda.synchronize()
            return rc, st, state.cpu().numpy(), msg.cpu().numpy(), count.cpu().numpy(), info.cpu().numpy()

        rc, st, state, msg, count, info = call(hip_alloc((n - 1) * MSG.itemsize))
        res["short_rc"] = rc
        res["short_untouched"] = bool(st == 0 and (state == 0).all() and (msg == 0xA5).all() and (count == -1).all()
                                      and (info == 0xA5).all())
        rc, st, state, msg, count, info = call(hip_alloc(n * MSG.itemsize))
        res["full_rc"], res["full_sync"] = rc, st
        res["full_count"] = [int(x) for x in count]
        res["full_bytes"] = bool((msg[:n] == 0x41).all() and (msg[n:] == 0xA5).all())
        res["full_consumed"] = int(state.view(STREAM_STATE)["consumed"][0])
        res["ok"] = (res["short_rc"] == ca.WSG_EINVAL and res["short_untouched"] and rc == 0 and st == 0
                     and res["full_count"] == [n, n] and res["full_bytes"] and res["full_consumed"] == n)
    finally:
        c.close()
        for p in blocks:
            hip.hipFree(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
