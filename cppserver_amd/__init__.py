"""cppserver_amd — MI355X-native WebSocket frame codec (CppServer's WS hot path).

The product is the C-ABI library ``_build/libwsg.so`` (include/wsg_capi.h):
gfx950 HIP kernels for batched header pack/unpack and payload mask/unmask.
This module is a thin ctypes binding over that ABI for Python callers and the
test-suite; torch is used only to own device memory and streams.

There is no CPU fallback: if the library or a GPU is missing, ``Codec``
raises instead of computing anything.
"""
import ctypes
import os

import numpy as np

from .layout import (  # noqa: F401  (re-exported)
    CB_CLOSE, CB_PING, CB_PONG, CB_RECEIVED, ECHO_REPLY, MSG, RECV_INFO, REPLY_SAME, SEND_DESC, STREAM_SPAN,
    STREAM_STATE, WS_BINARY, WS_CLOSE, WS_FIN, WS_PING, WS_PONG, WS_TEXT, WSG_EHIP, WSG_EINVAL, WSG_ENOMEM, WSG_ETRUNC,
    WSG_OK, UTF8_CLOSE, UTF8_EVERY, UTF8_TEXT, frame_plan, frame_size, frame_sizes, key_from_bytes, message_plan,
    reply_plan, utf8_plan,
    PROTO_ANY, PROTO_CLIENT, PROTO_SERVER, PROTO_STATE, PROTO_VERDICT, PV_CLOSE_CODE, PV_CLOSE_LEN, PV_CLOSED, PV_CONT,
    PV_CTRL_FRAGMENT, PV_CTRL_LONG, PV_DATA, PV_FRAME, PV_MASK, PV_NONE, PV_OPCODE, PV_RSV, PV_TOO_BIG, protocol_plan,
    PV_UTF8, checked_reply_plan, merge_verdicts, utf8_verdicts, utf8_wire_plan, validated_verdicts,
    AHEAD_CAP, ASSEMBLY_REFERENCE, ASSEMBLY_RFC, message_frames,
    UP_ACCEPTED, UP_BAD_CONNECTION, UP_BAD_HTTP, UP_BAD_UPGRADE, UP_BAD_VERSION, UP_EMPTY_KEY, UP_INCOMPLETE,
    UP_MISSING, UP_NOT_GET, UP_NOT_WEBSOCKET, UP_TOO_LONG, UPGRADE_DTYPE, UPGRADE_RESP_MAX, upgrade_plan,
    STREAM_READ, carry_plan,
    UC_ACCEPTED, UC_BAD_ACCEPT, UC_BAD_CONNECTION, UC_BAD_HTTP, UC_BAD_UPGRADE, UC_INCOMPLETE, UC_MISSING, UC_NOT_101,
    UC_TOO_LONG, UPGRADE_REPLY_DTYPE, upgrade_client_plan,
    CHAT_RELAY, CHAT_REPLY, relay_plan, relay_tables_bad,
)

_HERE = os.path.dirname(os.path.abspath(__file__))
# $WSG_LIB_PATH: another build of the same ABI for a one-off A/B check (tools/);
# unset, the in-tree library
LIB_PATH = os.environ.get("WSG_LIB_PATH") or os.path.join(_HERE, "_build", "libwsg.so")
ROOT = os.path.dirname(_HERE)
HEADERS = [os.path.join(ROOT, "include", "wsg_capi.h")]

_lib = None


class WSGError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib().wsg_strerror(code).decode() if _lib is not None else str(code)
        super().__init__("%s failed: %s (%d)" % (what or "wsg", msg, code))


def lib(path=None):
    """Load the HIP codec library; raise loudly if it was not built.

    `path` loads another build of the same ABI (A/B tuning); default is the
    in-tree library."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            "cppserver_amd: native library %s is missing; run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C cppserver_amd`). There is no CPU fallback." % p
        )
    L = ctypes.CDLL(p)
    vp, u32, u64, i32, sz, ci = (ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32,
                                 ctypes.c_size_t, ctypes.c_int)
    sig = {
        "wsg_abi_version": (ci, []),
        "wsg_strerror": (ctypes.c_char_p, [ci]),
        "wsg_create": (ci, [ci, ctypes.POINTER(vp)]),
        "wsg_destroy": (ci, [vp]),
        "wsg_sync": (ci, [vp, vp]),
        "wsg_stream": (vp, [vp]),
        "wsg_set_assembly": (ci, [vp, ci]),
        "wsg_get_assembly": (ci, [vp]),
        "wsg_decode_batch": (ci, [vp, vp, u64, vp, u32, vp, vp, vp]),
        "wsg_decode_messages": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, u64, vp, vp, vp, vp]),
        "wsg_frame_streams": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, vp]),
        "wsg_decode_streams": (ci, [vp, vp, u64, vp, u32, vp, vp, u32, vp, vp, u64, vp, vp, vp, ctypes.POINTER(u32),
                                    vp]),
        "wsg_reply_messages": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, ci, vp, vp, u64, vp, vp, vp, vp, vp, vp]),
        "wsg_reply_streams": (ci, [vp, vp, u64, vp, u32, vp, vp, u32, vp, vp, ci, vp, vp, u64, vp, vp, vp, vp, vp,
                                   ctypes.POINTER(u32), vp]),
        "wsg_reply_checked": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, u32, u64, vp, vp, ci, vp, vp, u64, vp, vp, vp,
                                   vp, vp, vp, vp, vp, vp]),
        "wsg_reply_checked_streams": (ci, [vp, vp, u64, vp, u32, vp, vp, u32, vp, vp, u32, u64, vp, ci, vp, vp, u64, vp,
                                           vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(u32), vp]),
        "wsg_reply_validated": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, u32, u64, vp, u32, vp, ci, vp, vp, u64, vp,
                                     vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "wsg_reply_validated_streams": (ci, [vp, vp, u64, vp, u32, vp, vp, u32, vp, vp, u32, u64, u32, vp, ci, vp, vp,
                                             u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(u32), vp]),
        "wsg_relay_validated": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, u32, u64, vp, u32, vp, ci, vp, vp, vp, vp,
                                     u32, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "wsg_relay_validated_streams": (ci, [vp, vp, u64, vp, u32, vp, vp, u32, vp, vp, u32, u64, u32, vp, ci, vp, vp,
                                             vp, vp, u32, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp,
                                             vp, vp, ctypes.POINTER(u32), vp]),
        "wsg_utf8_verdicts": (ci, [vp, vp, vp, u32, u32, vp, u32, vp, vp]),
        "wsg_check_utf8_wire": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp]),
        "wsg_check_utf8": (ci, [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp]),
        "wsg_utf8_valid_up_to": (u64, [vp, u64]),
        "wsg_check_protocol": (ci, [vp, vp, u64, vp, u32, vp, u32, vp, vp, u32, u64, vp, vp, vp]),
        "wsg_proto_judge": (ci, [vp, vp, vp, u32, u64, vp, ctypes.POINTER(ctypes.c_uint16)]),
        "wsg_upgrade_streams": (ci, [vp, vp, u64, vp, u32, u64, vp, vp, u64, vp, vp, vp]),
        "wsg_carry_streams": (ci, [vp, vp, u64, vp, u32, vp, vp, u64, vp, vp, u64, vp, vp, vp]),
        "wsg_upgrade_judge": (ci, [vp, u64, u64, vp, vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "wsg_upgrade_client_streams": (ci, [vp, vp, u64, vp, u32, vp, u64, vp, vp, vp]),
        "wsg_upgrade_requests": (ci, [vp, vp, u32, u32, vp, u32, vp, u64, vp]),
        "wsg_upgrade_client_judge": (ci, [vp, u64, vp, u64, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "wsg_upgrade_request": (ci, [vp, u32, u32, vp, vp]),
        "wsg_encode_batch": (ci, [vp, vp, vp, u32, vp, u64, vp, vp]),
        "wsg_fanout_encode": (ci, [vp, vp, u64, vp, u32, ctypes.c_uint8, ci, vp, u64, vp]),
        "wsg_fanout_encode_many": (ci, [vp, vp, vp, vp, vp, u32, vp, u32, ci, vp, u64, vp, vp]),
        "wsg_xor_host": (ci, [vp, vp, vp, sz, u32, u32]),
        "wsg_decode_batch_host": (ci, [vp, vp, u64, vp, u32, vp, vp]),
        "wsg_encode_batch_host": (ci, [vp, vp, u64, vp, u32, vp, u64, vp]),
        "wsg_host_alloc": (ci, [sz, ctypes.POINTER(vp)]),
        "wsg_host_free": (ci, [vp]),
        "wsg_frame_size": (u64, [ctypes.c_uint8, ci, u64, i32]),
        "wsg_header_pack": (ci, [ctypes.c_uint8, ci, u64, i32, u32, vp]),
        "wsg_header_unpack": (ci, [vp, u64, vp]),
        "wsg_ws_accept": (ci, [ctypes.c_char_p, sz, ctypes.c_char_p, sz]),
        "wsg_session_create": (ci, [vp, ctypes.POINTER(vp)]),
        "wsg_session_destroy": (ci, [vp]),
        "wsg_session_set_send_key": (ci, [vp, u32]),
        "wsg_session_prepare_send": (ci, [vp, ctypes.c_uint8, ci, vp, sz, i32, vp, sz, ctypes.POINTER(sz)]),
        "wsg_session_prepare_receive": (ci, [vp, vp, sz, vp, vp]),
        "wsg_session_required": (sz, [vp]),
        "wsg_session_clear": (ci, [vp]),
        "wsg_rx_create": (ci, [vp, ctypes.POINTER(vp)]),
        "wsg_rx_destroy": (ci, [vp]),
        "wsg_rx_feed": (ci, [vp, vp, vp, sz]),
        "wsg_rx_clear": (ci, [vp, vp]),
        "wsg_rx_forget": (ci, [vp, vp]),
        "wsg_rx_pending": (ci, [vp, ctypes.POINTER(u32), ctypes.POINTER(u64)]),
        "wsg_rx_set_devices": (ci, [vp, vp, ci]),
        "wsg_rx_flush": (ci, [vp, vp, vp, ctypes.POINTER(u32)]),
        "wsg_tx_create": (ci, [vp, ctypes.POINTER(vp)]),
        "wsg_tx_destroy": (ci, [vp]),
        "wsg_tx_queue": (ci, [vp, vp, ctypes.c_uint8, ci, vp, sz, i32]),
        "wsg_tx_forget": (ci, [vp, vp]),
        "wsg_tx_pending": (ci, [vp, ctypes.POINTER(u32), ctypes.POINTER(u64)]),
        "wsg_tx_set_devices": (ci, [vp, vp, ci]),
        "wsg_tx_flush": (ci, [vp, vp, vp, ctypes.POINTER(u32)]),
        "wsg_mgpu_create": (ci, [vp, ci, ctypes.POINTER(vp)]),
        "wsg_mgpu_unique_id": (ci, [vp]),
        "wsg_mgpu_create_rank": (ci, [ci, vp, ci, ci, ctypes.POINTER(vp)]),
        "wsg_mgpu_destroy": (ci, [vp]),
        "wsg_mgpu_info": (ci, [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]),
        "wsg_mgpu_ctx": (vp, [vp, ci]),
        "wsg_mgpu_shard_count": (u64, [u64, u32, ci, ci]),
        "wsg_mgpu_encode_gather": (ci, [vp, u64, u32, vp, vp, vp, vp, vp, vp, ci, vp, u64, vp, vp]),
        "wsg_decode_batch_host_multi": (ci, [vp, ci, vp, u64, vp, u32, vp, vp]),
        "wsg_encode_batch_host_multi": (ci, [vp, ci, vp, u64, vp, u32, vp, u64, vp]),
        "wsg_mgpu_decode_batch_host": (ci, [vp, vp, u64, vp, u32, vp, vp]),
        "wsg_mgpu_encode_batch_host": (ci, [vp, vp, u64, vp, u32, vp, u64, vp]),
        "wsg_timing_enable": (ci, [vp, ci]),
        "wsg_timing_read": (ci, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64), ci]),
        "wsg_timing_minmax": (ci, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
        "wsg_lane_stats": (ci, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(ci)]),
        "wsg_lane_events": (ci, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
    }
    for name, (res, args) in sig.items():
        if (path is not None or os.environ.get("WSG_LIB_PATH")) and not hasattr(L, name):
            continue   # an older A/B build of the library (tools/): bind what it has
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = L
    return L


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(rc, what):
    if rc != 0:
        raise WSGError(rc, what)


# ---- host helpers (pure host functions of the ABI; no device needed) ------
def header_pack(opcode, mask, length, status=0, key=0):
    buf = (ctypes.c_uint8 * 16)()
    n = lib().wsg_header_pack(opcode, 1 if mask else 0, length, status, key, buf)
    if n < 0:
        raise WSGError(n, "wsg_header_pack")
    return bytes(buf[:n])


def header_unpack(data):
    data = bytes(data)
    info = np.zeros(1, dtype=RECV_INFO)
    rc = lib().wsg_header_unpack(data, len(data), _np_ptr(info))
    return rc, info[0]


def utf8_valid_up_to(data):
    """wsg_utf8_valid_up_to: the length of the longest well-formed UTF-8
    prefix of ``data`` (the host helper built from the rule the kernel runs)."""
    data = bytes(data)
    return int(lib().wsg_utf8_valid_up_to(data, len(data)))


def proto_judge(info, wire, before, role=PROTO_ANY, max_message=0):
    """wsg_proto_judge: one frame judged on the host by the rule the kernel
    runs.  ``info``: one RECV_INFO record; ``wire``: the bytes its payload_off
    indexes (a close frame's status is read from them; None: no wire);
    ``before``: one PROTO_STATE record, or (bytes, open).  Returns (code,
    status, after): the WSG_PV_* code (0: none), the close status that goes
    with it and the PROTO_STATE behind the frame."""
    rec = np.zeros(1, dtype=RECV_INFO)
    rec[0] = info
    st = np.zeros(2, dtype=PROTO_STATE)
    if isinstance(before, tuple):
        st["bytes"][0], st["open"][0] = before
    else:
        st[0] = before
    if isinstance(wire, (bytes, bytearray)):
        wire = np.frombuffer(bytes(wire), dtype=np.uint8)
    buf = None if wire is None else np.ascontiguousarray(wire, dtype=np.uint8)
    status = ctypes.c_uint16(0)
    rc = lib().wsg_proto_judge(_np_ptr(rec), None if buf is None else _np_ptr(buf), _np_ptr(st[:1]), int(role),
                               int(max_message), _np_ptr(st[1:]), ctypes.byref(status))
    if rc < 0:
        raise WSGError(rc, "wsg_proto_judge")
    return rc, int(status.value), st[1].copy()


def upgrade_judge(data, max_request=0, resp_cap=UPGRADE_RESP_MAX):
    """wsg_upgrade_judge: one connection's first bytes judged on the host by
    the rule the kernels run.  Returns (rc, record, resp, consumed, need): the
    call's status (WSG_ENOMEM when the response needs more than ``resp_cap``
    bytes), one UPGRADE_DTYPE record, the response bytes, and the span's
    outputs."""
    data = bytes(data)
    rec = np.zeros(1, dtype=UPGRADE_DTYPE)
    resp = np.zeros(max(int(resp_cap), 1), dtype=np.uint8)
    consumed, need = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().wsg_upgrade_judge(data, len(data), int(max_request), _np_ptr(rec), _np_ptr(resp) if resp_cap else None,
                                 int(resp_cap), ctypes.byref(consumed), ctypes.byref(need))
    if rc not in (WSG_OK, WSG_ENOMEM):
        raise WSGError(rc, "wsg_upgrade_judge")
    sent = resp[: int(rec["resp_len"][0])].tobytes() if rc == WSG_OK else b""
    return rc, rec[0].copy(), sent, int(consumed.value), int(need.value)


def upgrade_client_judge(data, nonce, max_response=0):
    """wsg_upgrade_client_judge: one client connection's first bytes judged on
    the host, against the 16-byte ``nonce``, by the rule the kernels run.
    Returns (record, consumed, need): one UPGRADE_REPLY_DTYPE record and the
    span's outputs."""
    data, nonce = bytes(data), bytes(nonce)
    if len(nonce) != 16:
        raise WSGError(WSG_EINVAL, "upgrade_client_judge: the nonce has 16 bytes")
    rec = np.zeros(1, dtype=UPGRADE_REPLY_DTYPE)
    consumed, need = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().wsg_upgrade_client_judge(data, len(data), nonce, int(max_response), _np_ptr(rec),
                                          ctypes.byref(consumed), ctypes.byref(need)), "wsg_upgrade_client_judge")
    return rec[0].copy(), int(consumed.value), int(need.value)


def upgrade_request(tpl, key_at, nonce):
    """wsg_upgrade_request: the request template with Base64(nonce) in its
    24-byte hole at ``key_at``."""
    tpl, nonce = bytes(tpl), bytes(nonce)
    if len(nonce) != 16:
        raise WSGError(WSG_EINVAL, "upgrade_request: the nonce has 16 bytes")
    out = ctypes.create_string_buffer(max(len(tpl), 1))
    _check(lib().wsg_upgrade_request(tpl, len(tpl), int(key_at), nonce, out), "wsg_upgrade_request")
    return out.raw[: len(tpl)]


class _Pinned:
    """Owner of a wsg_host_alloc block; freed when the last view dies."""

    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        _check(lib().wsg_host_alloc(nbytes, ctypes.byref(self.ptr)), "wsg_host_alloc")

    def __del__(self):
        if self.ptr:
            lib().wsg_host_free(self.ptr)
            self.ptr = None


def pinned_empty(nbytes, dtype=np.uint8):
    """numpy array in page-locked host memory (DMA without staging)."""
    owner = _Pinned(max(int(nbytes), 1))
    buf = (ctypes.c_uint8 * max(int(nbytes), 1)).from_address(owner.ptr.value)
    buf._owner = owner   # the numpy view keeps buf alive, buf keeps the block alive
    return np.frombuffer(buf, dtype=np.uint8)[: int(nbytes)].view(dtype)


def abi_frame_size(opcode, mask, length, status=0):
    return int(lib().wsg_frame_size(opcode, 1 if mask else 0, length, status))


class Codec:
    """A wsg_ctx bound to one HIP device.

    Batch methods take torch CUDA (HIP) tensors resident in HBM and run
    asynchronously on ``stream`` (default: torch's current stream); call
    :meth:`sync` before reading results on the host.
    """

    def __init__(self, device=0, lib_path=None):
        import torch

        self._torch = torch
        self._L = lib(lib_path)
        if not torch.cuda.is_available():
            raise WSGError(WSG_EHIP, "Codec: no HIP device visible")
        self.device = torch.device("cuda", device)
        ctx = ctypes.c_void_p()
        _check(self._L.wsg_create(device, ctypes.byref(ctx)), "wsg_create")
        self._ctx = ctx

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.wsg_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    # -- streams / sync ----------------------------------------------------
    def _stream(self, stream):
        if stream is None:
            stream = self._torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))

    def own_stream(self):
        """The context's own non-blocking stream (wsg_stream) as a torch
        stream: pass it as ``stream`` or enter it with torch.cuda.stream().
        It lives as long as the context."""
        return self._torch.cuda.ExternalStream(self._L.wsg_stream(self._ctx), device=self.device)

    def sync(self, stream=None):
        """Synchronize and raise WSGError on a latched data-dependent error."""
        _check(self._L.wsg_sync(self._ctx, self._stream(stream)), "wsg_sync")

    def sync_status(self, stream=None):
        return self._L.wsg_sync(self._ctx, self._stream(stream))

    # -- the assembly rule ---------------------------------------------------
    def set_assembly(self, mode):
        """wsg_set_assembly: ASSEMBLY_REFERENCE (the default) or ASSEMBLY_RFC
        for every later call that runs the message plan (decode_messages,
        reply_messages, check_utf8_wire, reply_checked, reply_validated and
        their _streams forms)."""
        _check(self._L.wsg_set_assembly(self._ctx, int(mode)), "wsg_set_assembly")

    @property
    def assembly(self):
        """The mode wsg_get_assembly reports."""
        return int(self._L.wsg_get_assembly(self._ctx))

    # -- batch decode (unmask) ----------------------------------------------
    def decode_batch(self, wire, frame_start, out=None, info=None, stream=None):
        """Unmask every frame of ``wire`` (uint8 CUDA tensor) whose starts are
        ``frame_start`` (int64 CUDA tensor).  Returns (out, info_bytes)."""
        t = self._torch
        n = int(frame_start.numel())
        if out is None:
            out = t.empty_like(wire)
        if info is None:
            info = t.empty(max(n, 1) * RECV_INFO.itemsize, dtype=t.uint8, device=wire.device)
        rc = self._L.wsg_decode_batch(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                      ctypes.c_void_p(frame_start.data_ptr()), n,
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                                      self._stream(stream))
        _check(rc, "wsg_decode_batch")
        return out, info

    # -- batch decode to messages (unmask + assemble + pack) -----------------
    def decode_messages(self, wire, frame_start, stream_first, state=None, msg=None, msg_cap=None, stream=None,
                        msgs=None, count=None, info=None):
        """wsg_decode_messages: the frames of ``wire`` (as decode_batch),
        grouped into streams by ``stream_first`` (int32 CUDA tensor of
        n_streams + 1 frame indices), assembled into messages and packed
        densely.  ``state``: uint8 CUDA tensor of n_streams * 8 bytes
        (STREAM_STATE; None: zeros), updated in place.  Returns (msg, msgs,
        count, state, info): the message bytes, the MSG table bytes (room for n
        records, count[0] valid), count int64[2] = [messages, bytes used], the
        new state and the RECV_INFO bytes.  ``msg_cap`` defaults to the wire's
        length, which always suffices."""
        t = self._torch
        n = int(frame_start.numel())
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "decode_messages: stream_first must hold n_streams + 1 32-bit indices")
        dev = wire.device
        if state is None:
            state = t.zeros(max(ns, 1) * STREAM_STATE.itemsize, dtype=t.uint8, device=dev)
        if msg_cap is None:
            msg_cap = int(wire.numel()) if msg is None else int(msg.numel())
        cap = int(msg_cap)
        if msg is None:
            msg = t.empty(max(cap, 16), dtype=t.uint8, device=dev)
        if msgs is None:
            msgs = t.empty(max(n, 1) * MSG.itemsize, dtype=t.uint8, device=dev)
        if count is None:
            count = t.empty(2, dtype=t.int64, device=dev)
        if info is None:
            info = t.empty(max(n, 1) * RECV_INFO.itemsize, dtype=t.uint8, device=dev)
        if (cap > int(msg.numel()) or int(state.numel()) < ns * STREAM_STATE.itemsize
                or int(msgs.numel()) < n * MSG.itemsize or int(info.numel()) < n * RECV_INFO.itemsize):
            raise WSGError(WSG_EINVAL, "decode_messages: a buffer is smaller than the batch needs")
        rc = self._L.wsg_decode_messages(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                         ctypes.c_void_p(frame_start.data_ptr()), n,
                                         ctypes.c_void_p(stream_first.data_ptr()), ns,
                                         ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(msg.data_ptr()), cap,
                                         ctypes.c_void_p(msgs.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                         ctypes.c_void_p(info.data_ptr()), self._stream(stream))
        _check(rc, "wsg_decode_messages")
        return msg, msgs, count, state, info

    # -- UTF-8 of text messages and close reasons -----------------------------
    def check_utf8(self, msg, msgs, count, which=UTF8_TEXT | UTF8_CLOSE, msg_cap=None, msg_room=None, valid=None,
                   result=None, stream=None):
        """wsg_check_utf8 over what decode_messages / decode_streams returned:
        ``msg`` the message bytes, ``msgs`` the MSG table bytes, ``count``
        int64[2] (read on the device: no synchronisation needed after the
        decode on the same stream).  ``which``: UTF8_* bits.  ``msg_cap``
        defaults to msg's length and ``msg_room`` to the records msgs has room
        for.  Returns (valid, result): int64[msg_room], valid[m] = the length
        of message m's longest well-formed prefix (its len when it is valid or
        not checked), written for m < min(count[0], msg_room); and int64[4] =
        [invalid messages, the lowest of them or -1, messages checked, bytes
        checked]."""
        t = self._torch
        dev = msg.device
        if msg_cap is None:
            msg_cap = int(msg.numel())
        if msg_room is None:
            msg_room = int(msgs.numel()) // MSG.itemsize if valid is None else int(valid.numel())
        cap, room = int(msg_cap), int(msg_room)
        if valid is None:
            valid = t.empty(max(room, 1), dtype=t.int64, device=dev)
        if result is None:
            result = t.empty(4, dtype=t.int64, device=dev)
        if (cap > int(msg.numel()) or int(msgs.numel()) < room * MSG.itemsize or int(valid.numel()) < room
                or valid.element_size() != 8 or int(count.numel()) < 2 or count.element_size() != 8
                or int(result.numel()) < 4 or result.element_size() != 8):
            raise WSGError(WSG_EINVAL, "check_utf8: a buffer is smaller than the batch needs")
        rc = self._L.wsg_check_utf8(self._ctx, ctypes.c_void_p(msg.data_ptr()), cap, ctypes.c_void_p(msgs.data_ptr()),
                                    ctypes.c_void_p(count.data_ptr()), room, int(which),
                                    ctypes.c_void_p(valid.data_ptr()), ctypes.c_void_p(result.data_ptr()),
                                    self._stream(stream))
        _check(rc, "wsg_check_utf8")
        return valid, result

    def check_utf8_wire(self, wire, frame_start, stream_first, state=None, which=UTF8_TEXT | UTF8_CLOSE, msgs=None,
                        count=None, info=None, valid=None, result=None, stream=None):
        """wsg_check_utf8_wire: check_utf8 over the messages of a frame table,
        read from the masked wire (no message buffer).  ``wire`` /
        ``frame_start`` / ``stream_first`` / ``state`` as decode_messages, but
        ``state`` is only read.  Returns (valid, result, msgs, count, info):
        valid int64[n] and result int64[4] as check_utf8 returns them for the
        dense layout of the same messages, and the MSG table bytes, count
        int64[2] and the RECV_INFO bytes as decode_messages writes them."""
        t = self._torch
        n = int(frame_start.numel())
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "check_utf8_wire: stream_first must hold n_streams + 1 32-bit indices")
        dev = wire.device
        if state is None:
            state = t.zeros(max(ns, 1) * STREAM_STATE.itemsize, dtype=t.uint8, device=dev)
        if msgs is None:
            msgs = t.empty(max(n, 1) * MSG.itemsize, dtype=t.uint8, device=dev)
        if count is None:
            count = t.empty(2, dtype=t.int64, device=dev)
        if info is None:
            info = t.empty(max(n, 1) * RECV_INFO.itemsize, dtype=t.uint8, device=dev)
        if valid is None:
            valid = t.empty(max(n, 1), dtype=t.int64, device=dev)
        if result is None:
            result = t.empty(4, dtype=t.int64, device=dev)
        if (int(state.numel()) < ns * STREAM_STATE.itemsize or int(msgs.numel()) < n * MSG.itemsize
                or int(info.numel()) < n * RECV_INFO.itemsize or int(count.numel()) < 2 or count.element_size() != 8
                or valid.element_size() != 8 or int(result.numel()) < 4 or result.element_size() != 8):
            raise WSGError(WSG_EINVAL, "check_utf8_wire: a buffer is smaller than the batch needs")
        p = ctypes.c_void_p
        rc = self._L.wsg_check_utf8_wire(self._ctx, p(wire.data_ptr()), wire.numel(), p(frame_start.data_ptr()), n,
                                         p(stream_first.data_ptr()), ns, p(state.data_ptr()), int(which),
                                         p(msgs.data_ptr()), p(count.data_ptr()), p(info.data_ptr()),
                                         p(valid.data_ptr()), p(result.data_ptr()), self._stream(stream))
        _check(rc, "wsg_check_utf8_wire")
        return valid, result, msgs, count, info

    # -- the frame-sequence rules of RFC 6455 ----------------------------------
    def check_protocol(self, wire, info, n, stream_first, proto=None, role=PROTO_ANY, max_message=0, state=None,
                       verdict=None, result=None, stream=None):
        """wsg_check_protocol over what a decode left on the device: ``wire``
        the batch's bytes, ``info`` the RECV_INFO bytes of its ``n`` frames,
        ``stream_first`` int32[n_streams + 1] (no synchronisation needed after
        the decode on the same stream).  ``proto``: uint8 CUDA tensor of
        n_streams * 16 bytes (PROTO_STATE; None: zeros), each stream's state
        before its first frame, updated in place to the state after its last
        frame, or, with ``state`` (decode_messages' STREAM_STATE bytes), after
        its last consumed frame.  ``role``: PROTO_*; ``max_message``: 0 for no
        limit.  Returns (verdict, proto, result): the PROTO_VERDICT bytes (8
        per stream, all 0xFF for a stream with no terminal frame), the new
        states and int64[3] = [streams that violate, the lowest of them or
        -1, streams closed cleanly]."""
        t = self._torch
        n = int(n)
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "check_protocol: stream_first must hold n_streams + 1 32-bit indices")
        dev = info.device
        if proto is None:
            proto = t.zeros(max(ns, 1) * PROTO_STATE.itemsize, dtype=t.uint8, device=dev)
        if verdict is None:
            verdict = t.empty(max(ns, 1) * PROTO_VERDICT.itemsize, dtype=t.uint8, device=dev)
        if result is None:
            result = t.empty(3, dtype=t.int64, device=dev)
        if (int(info.numel()) * info.element_size() < n * RECV_INFO.itemsize
                or int(proto.numel()) * proto.element_size() < ns * PROTO_STATE.itemsize
                or int(verdict.numel()) * verdict.element_size() < ns * PROTO_VERDICT.itemsize
                or (state is not None and int(state.numel()) * state.element_size() < ns * STREAM_STATE.itemsize)
                or int(result.numel()) < 3 or result.element_size() != 8):
            raise WSGError(WSG_EINVAL, "check_protocol: a buffer is smaller than the batch needs")
        rc = self._L.wsg_check_protocol(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                        ctypes.c_void_p(info.data_ptr()), n,
                                        ctypes.c_void_p(stream_first.data_ptr()), ns,
                                        ctypes.c_void_p(state.data_ptr()) if state is not None else None,
                                        ctypes.c_void_p(proto.data_ptr()), int(role), int(max_message),
                                        ctypes.c_void_p(verdict.data_ptr()), ctypes.c_void_p(result.data_ptr()),
                                        self._stream(stream))
        _check(rc, "wsg_check_protocol")
        return verdict, proto, result

    # -- the device framer (raw stream bytes -> frame table -> messages) ------
    def _frame_args(self, what, wire, spans, frame_start, frame_cap, stream_first):
        t = self._torch
        ns = int(spans.numel()) // STREAM_SPAN.itemsize
        if spans.element_size() != 1 or int(spans.numel()) != ns * STREAM_SPAN.itemsize:
            raise WSGError(WSG_EINVAL, "%s: spans must be uint8, n_streams * 32 bytes" % what)
        dev = wire.device
        if frame_cap is None:   # every frame has at least two bytes
            frame_cap = int(wire.numel()) // 2 if frame_start is None else int(frame_start.numel())
        cap = int(frame_cap)
        if frame_start is None:
            frame_start = t.empty(max(cap, 1), dtype=t.int64, device=dev)
        if stream_first is None:
            stream_first = t.empty(ns + 1, dtype=t.int32, device=dev)
        if (cap > int(frame_start.numel()) or frame_start.element_size() != 8 or stream_first.element_size() != 4
                or int(stream_first.numel()) < ns + 1 or cap > 0xFFFFFFFF):
            raise WSGError(WSG_EINVAL, "%s: a buffer is smaller than the batch needs" % what)
        return ns, cap, frame_start, stream_first

    def frame_streams(self, wire, spans, frame_start=None, frame_cap=None, stream_first=None, count=None,
                      stream=None):
        """wsg_frame_streams: the frame boundaries of the streams ``spans``
        (uint8 CUDA tensor of n_streams * 32 bytes, STREAM_SPAN: off and len
        in, consumed and need out, in place) of ``wire``.  Returns
        (frame_start, stream_first, count): int64[frame_cap] wire offsets
        (count[0] valid), int32[n_streams + 1] and count int64[2] = [frames,
        bytes in whole frames].  ``frame_cap`` defaults to the room of
        ``frame_start``, or to wire bytes / 2, which always suffices."""
        t = self._torch
        ns, cap, frame_start, stream_first = self._frame_args("frame_streams", wire, spans, frame_start, frame_cap,
                                                              stream_first)
        if count is None:
            count = t.empty(2, dtype=t.int64, device=wire.device)
        rc = self._L.wsg_frame_streams(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                       ctypes.c_void_p(spans.data_ptr()), ns,
                                       ctypes.c_void_p(frame_start.data_ptr()), cap,
                                       ctypes.c_void_p(stream_first.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                       self._stream(stream))
        _check(rc, "wsg_frame_streams")
        return frame_start, stream_first, count

    def upgrade_streams(self, wire, spans, resp_cap=None, max_request=0, stream=None, up=None, resp=None,
                        resp_off=None, count=None):
        """wsg_upgrade_streams: the upgrade request at the head of every stream
        of ``spans`` (as in frame_streams: consumed and need out, in place)
        judged on the device.  Returns (up, resp, resp_off, count): uint8
        [n_streams * 32] UPGRADE_DTYPE records, the response bytes in stream
        order (``resp_cap`` bytes of room; default n_streams *
        UPGRADE_RESP_MAX, which always suffices), int64[n_streams + 1] their
        exclusive prefix, and count int64[4] = [accepted, answered with a
        400, incomplete, response bytes].  A total above ``resp_cap`` latches
        WSG_ENOMEM (sync) with no byte of ``resp`` written."""
        t = self._torch
        ns = int(spans.numel()) // STREAM_SPAN.itemsize
        if spans.element_size() != 1 or int(spans.numel()) != ns * STREAM_SPAN.itemsize:
            raise WSGError(WSG_EINVAL, "upgrade_streams: spans must be uint8, n_streams * 32 bytes")
        dev = wire.device
        if resp_cap is None:
            resp_cap = ns * UPGRADE_RESP_MAX if resp is None else int(resp.numel())
        cap = int(resp_cap)
        if up is None:
            up = t.empty(max(ns, 1) * UPGRADE_DTYPE.itemsize, dtype=t.uint8, device=dev)
        if resp is None:
            resp = t.empty(max(cap, 1), dtype=t.uint8, device=dev)
        if resp_off is None:
            resp_off = t.empty(ns + 1, dtype=t.int64, device=dev)
        if count is None:
            count = t.empty(4, dtype=t.int64, device=dev)
        if (int(up.numel()) * up.element_size() < ns * UPGRADE_DTYPE.itemsize or cap > int(resp.numel())
                or resp.element_size() != 1 or resp_off.element_size() != 8 or int(resp_off.numel()) < ns + 1
                or count.element_size() != 8 or int(count.numel()) < 4):
            raise WSGError(WSG_EINVAL, "upgrade_streams: a buffer is smaller than the batch needs")
        rc = self._L.wsg_upgrade_streams(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                         ctypes.c_void_p(spans.data_ptr()), ns, int(max_request),
                                         ctypes.c_void_p(up.data_ptr()), ctypes.c_void_p(resp.data_ptr()), cap,
                                         ctypes.c_void_p(resp_off.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                         self._stream(stream))
        _check(rc, "wsg_upgrade_streams")
        return up, resp, resp_off, count

    def upgrade_client_streams(self, wire, spans, nonces, max_response=0, stream=None, up=None, count=None):
        """wsg_upgrade_client_streams: the upgrade response at the head of
        every stream of ``spans`` (consumed and need out, in place) judged on
        the device against ``nonces`` (uint8, 16 bytes a stream).  Returns
        (up, count): uint8[n_streams * 32] UPGRADE_REPLY_DTYPE records and
        count int64[3] = [accepted, whole but not accepted, incomplete]."""
        t = self._torch
        ns = int(spans.numel()) // STREAM_SPAN.itemsize
        if spans.element_size() != 1 or int(spans.numel()) != ns * STREAM_SPAN.itemsize:
            raise WSGError(WSG_EINVAL, "upgrade_client_streams: spans must be uint8, n_streams * 32 bytes")
        if nonces.element_size() != 1 or int(nonces.numel()) < 16 * ns:
            raise WSGError(WSG_EINVAL, "upgrade_client_streams: nonces must be uint8, 16 bytes a stream")
        dev = wire.device
        if up is None:
            up = t.empty(max(ns, 1) * UPGRADE_REPLY_DTYPE.itemsize, dtype=t.uint8, device=dev)
        if count is None:
            count = t.empty(3, dtype=t.int64, device=dev)
        if (int(up.numel()) * up.element_size() < ns * UPGRADE_REPLY_DTYPE.itemsize or count.element_size() != 8
                or int(count.numel()) < 3):
            raise WSGError(WSG_EINVAL, "upgrade_client_streams: a buffer is smaller than the batch needs")
        rc = self._L.wsg_upgrade_client_streams(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                                ctypes.c_void_p(spans.data_ptr()), ns,
                                                ctypes.c_void_p(nonces.data_ptr()), int(max_response),
                                                ctypes.c_void_p(up.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                                self._stream(stream))
        _check(rc, "wsg_upgrade_client_streams")
        return up, count

    def upgrade_requests(self, tpl, key_at, nonces, req=None, req_cap=None, stream=None):
        """wsg_upgrade_requests: one request per 16 bytes of ``nonces``
        (uint8), each the template ``tpl`` (uint8, a 24-byte hole at
        ``key_at``) with Base64 of its nonce in the hole.  Returns the
        requests back to back (``req_cap`` bytes of room; default exactly
        what they need)."""
        t = self._torch
        n = int(nonces.numel()) // 16
        tpl_len = int(tpl.numel())
        if tpl.element_size() != 1 or nonces.element_size() != 1 or int(nonces.numel()) != 16 * n:
            raise WSGError(WSG_EINVAL, "upgrade_requests: tpl and nonces must be uint8, 16 bytes a nonce")
        if req_cap is None:
            req_cap = n * tpl_len if req is None else int(req.numel())
        if req is None:
            req = t.empty(max(int(req_cap), 1), dtype=t.uint8, device=tpl.device)
        if req.element_size() != 1 or int(req_cap) > int(req.numel()):
            raise WSGError(WSG_EINVAL, "upgrade_requests: req is smaller than req_cap")
        rc = self._L.wsg_upgrade_requests(self._ctx, ctypes.c_void_p(tpl.data_ptr()), tpl_len, int(key_at),
                                          ctypes.c_void_p(nonces.data_ptr()), n, ctypes.c_void_p(req.data_ptr()),
                                          int(req_cap), self._stream(stream))
        _check(rc, "wsg_upgrade_requests")
        return req

    def carry_streams(self, wire, spans, new, reads, close_off=None, next=None, next_cap=None, next_spans=None,
                      count=None, stream=None):
        """wsg_carry_streams: the next round's wire and span table from the
        last round's ``wire`` and ``spans`` (uint8, n_streams * 32 bytes, as
        that round's calls left them) and the bytes just read: ``new`` with
        ``reads`` (uint8, n_streams * 16 bytes, STREAM_READ; None: no stream
        has new bytes).  ``close_off`` (None, or n_streams words as
        reply_checked / reply_validated write them) drops the streams whose
        word is not 2**64 - 1.  ``wire`` and ``new`` may be None for no bytes.
        Returns (next, next_spans, count): the wire (``next_cap`` bytes of
        room; default what always suffices), its STREAM_SPAN records and count
        int64[4] = [bytes of next, tail bytes, new bytes, streams dropped].  A
        total above ``next_cap`` latches WSG_ENOMEM (sync) with no byte of
        ``next`` written."""
        t = self._torch
        ns = int(spans.numel()) // STREAM_SPAN.itemsize
        if spans.element_size() != 1 or int(spans.numel()) != ns * STREAM_SPAN.itemsize:
            raise WSGError(WSG_EINVAL, "carry_streams: spans must be uint8, n_streams * 32 bytes")
        dev = spans.device
        wire_len = 0 if wire is None else int(wire.numel())
        new_len = 0 if new is None else int(new.numel())
        if next_cap is None:   # a stream adds less than 16 bytes of padding to its bytes
            next_cap = wire_len + new_len + 16 * ns if next is None else int(next.numel())
        cap = int(next_cap)
        if next is None:
            next = t.empty(max(cap, 16), dtype=t.uint8, device=dev)
        if next_spans is None:
            next_spans = t.empty(max(ns, 1) * STREAM_SPAN.itemsize, dtype=t.uint8, device=dev)
        if count is None:
            count = t.empty(4, dtype=t.int64, device=dev)
        if (cap > int(next.numel()) or next.element_size() != 1
                or int(next_spans.numel()) * next_spans.element_size() < ns * STREAM_SPAN.itemsize
                or (reads is not None and int(reads.numel()) * reads.element_size() < ns * STREAM_READ.itemsize)
                or (close_off is not None and (close_off.element_size() != 8 or int(close_off.numel()) < ns))
                or count.element_size() != 8 or int(count.numel()) < 4):
            raise WSGError(WSG_EINVAL, "carry_streams: a buffer is smaller than the batch needs")

        def ptr(x):
            return ctypes.c_void_p(None if x is None else x.data_ptr())

        rc = self._L.wsg_carry_streams(self._ctx, ptr(wire), wire_len, ptr(spans), ns, ptr(close_off), ptr(new),
                                       new_len, ptr(reads), ptr(next), cap, ptr(next_spans), ptr(count),
                                       self._stream(stream))
        _check(rc, "wsg_carry_streams")
        return next, next_spans, count

    def decode_streams(self, wire, spans, state=None, frame_start=None, frame_cap=None, stream_first=None,
                       msg=None, msg_cap=None, stream=None, msgs=None, count=None, info=None):
        """wsg_decode_streams: frame_streams, then decode_messages over the
        frames it found (one stream synchronisation between the two), then
        every span's consumed lowered to the stream's first tail frame.
        ``spans`` as frame_streams, ``state`` / ``msg`` / ``msg_cap`` /
        ``msgs`` / ``count`` / ``info`` as decode_messages with room for
        ``frame_cap`` frames (the default, wire bytes / 2, makes ``msgs`` and
        ``info`` 36 times the wire: give a ``frame_cap`` for anything large).
        Returns (msg, msgs, count, state, info, frame_start, stream_first,
        n_frames)."""
        t = self._torch
        ns, cap, frame_start, stream_first = self._frame_args("decode_streams", wire, spans, frame_start, frame_cap,
                                                              stream_first)
        dev = wire.device
        if state is None:
            state = t.zeros(max(ns, 1) * STREAM_STATE.itemsize, dtype=t.uint8, device=dev)
        if msg_cap is None:
            msg_cap = int(wire.numel()) if msg is None else int(msg.numel())
        mcap = int(msg_cap)
        if msg is None:
            msg = t.empty(max(mcap, 16), dtype=t.uint8, device=dev)
        if msgs is None:
            msgs = t.empty(max(cap, 1) * MSG.itemsize, dtype=t.uint8, device=dev)
        if count is None:
            count = t.empty(2, dtype=t.int64, device=dev)
        if info is None:
            info = t.empty(max(cap, 1) * RECV_INFO.itemsize, dtype=t.uint8, device=dev)
        if (mcap > int(msg.numel()) or int(state.numel()) < ns * STREAM_STATE.itemsize
                or int(msgs.numel()) < cap * MSG.itemsize or int(info.numel()) < cap * RECV_INFO.itemsize):
            raise WSGError(WSG_EINVAL, "decode_streams: a buffer is smaller than the batch needs")
        n = ctypes.c_uint32()
        rc = self._L.wsg_decode_streams(self._ctx, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                        ctypes.c_void_p(spans.data_ptr()), ns, ctypes.c_void_p(state.data_ptr()),
                                        ctypes.c_void_p(frame_start.data_ptr()), cap,
                                        ctypes.c_void_p(stream_first.data_ptr()), ctypes.c_void_p(msg.data_ptr()),
                                        mcap, ctypes.c_void_p(msgs.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                        ctypes.c_void_p(info.data_ptr()), ctypes.byref(n), self._stream(stream))
        _check(rc, "wsg_decode_streams")
        return msg, msgs, count, state, info, frame_start, stream_first, n.value

    # -- replies (frames -> messages -> frames to send, payload moved once) ----
    def _reply_args(self, what, wire, n, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply, state,
                    msgs, count, info):
        t = self._torch
        dev = wire.device
        rule = bytes(int(x) for x in reply_op)
        if len(rule) != 5:
            raise WSGError(WSG_EINVAL, "%s: reply_op must hold five bytes (indexed by CB_*)" % what)
        if send_keys is not None and (send_keys.element_size() != 4 or int(send_keys.numel()) < ns):
            raise WSGError(WSG_EINVAL, "%s: send_keys must hold n_streams 32-bit keys" % what)
        if reply_cap is None:   # a reply adds at most 16 bytes to its data, every frame spent 2 on its header
            reply_cap = int(wire.numel()) + 14 * n if reply is None else int(reply.numel())
        cap = int(reply_cap)
        if reply is None:
            reply = t.empty(max(cap, 16), dtype=t.uint8, device=dev)
        if reply_off is None:
            reply_off = t.empty(n + 1, dtype=t.int64, device=dev)
        if stream_reply is None:
            stream_reply = t.empty(ns + 1, dtype=t.int64, device=dev)
        if state is None:
            state = t.zeros(max(ns, 1) * STREAM_STATE.itemsize, dtype=t.uint8, device=dev)
        if msgs is None:
            msgs = t.empty(max(n, 1) * MSG.itemsize, dtype=t.uint8, device=dev)
        if count is None:
            count = t.empty(4, dtype=t.int64, device=dev)
        if info is None:
            info = t.empty(max(n, 1) * RECV_INFO.itemsize, dtype=t.uint8, device=dev)
        if (cap > int(reply.numel()) or int(reply_off.numel()) < n + 1 or reply_off.element_size() != 8
                or int(stream_reply.numel()) < ns + 1 or stream_reply.element_size() != 8
                or int(count.numel()) < 4 or count.element_size() != 8
                or int(state.numel()) < ns * STREAM_STATE.itemsize or int(msgs.numel()) < n * MSG.itemsize
                or int(info.numel()) < n * RECV_INFO.itemsize):
            raise WSGError(WSG_EINVAL, "%s: a buffer is smaller than the batch needs" % what)
        return rule, cap, reply, reply_off, stream_reply, state, msgs, count, info

    def reply_messages(self, wire, frame_start, stream_first, reply_op=ECHO_REPLY, mask=False, send_keys=None,
                       state=None, reply=None, reply_cap=None, stream=None, reply_off=None, stream_reply=None,
                       msgs=None, count=None, info=None):
        """wsg_reply_messages: the frames of ``wire`` as decode_messages takes
        them, answered: ``reply_op`` (five bytes by CB_*: 0 none, REPLY_SAME,
        or the reply's first header byte), ``mask``, ``send_keys`` (int32 CUDA
        tensor, one little-endian key per stream; None: all 0).  Returns
        (reply, reply_off, stream_reply, msgs, count, state, info): the reply
        frames back to back, int64[n + 1] offsets per message (count[0] + 1
        valid), int64[n_streams + 1] offsets per stream, the MSG table bytes,
        count int64[4] = [messages, bytes of the dense layout, reply bytes,
        reply frames], the new state and the RECV_INFO bytes.  ``reply_cap``
        defaults to wire bytes + 14 * n, which always suffices."""
        n = int(frame_start.numel())
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "reply_messages: stream_first must hold n_streams + 1 32-bit indices")
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "reply_messages", wire, n, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply, state, msgs,
            count, info)
        p = ctypes.c_void_p
        rc = self._L.wsg_reply_messages(self._ctx, p(wire.data_ptr()), wire.numel(), p(frame_start.data_ptr()), n,
                                        p(stream_first.data_ptr()), ns, p(state.data_ptr()), rule, 1 if mask else 0,
                                        p(send_keys.data_ptr()) if send_keys is not None else None,
                                        p(reply.data_ptr()), cap, p(reply_off.data_ptr()), p(stream_reply.data_ptr()),
                                        p(msgs.data_ptr()), p(count.data_ptr()), p(info.data_ptr()),
                                        self._stream(stream))
        _check(rc, "wsg_reply_messages")
        return reply, reply_off, stream_reply, msgs, count, state, info

    def reply_streams(self, wire, spans, reply_op=ECHO_REPLY, mask=False, send_keys=None, state=None,
                      frame_start=None, frame_cap=None, stream_first=None, reply=None, reply_cap=None, stream=None,
                      reply_off=None, stream_reply=None, msgs=None, count=None, info=None):
        """wsg_reply_streams: frame_streams, then reply_messages over the
        frames it found (one stream synchronisation between the two), then
        every span's consumed lowered to the stream's first tail frame.
        Arguments as decode_streams and reply_messages, with room for
        ``frame_cap`` frames.  Returns (reply, reply_off, stream_reply, msgs,
        count, state, info, frame_start, stream_first, n_frames)."""
        ns, fcap, frame_start, stream_first = self._frame_args("reply_streams", wire, spans, frame_start, frame_cap,
                                                               stream_first)
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "reply_streams", wire, fcap, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply, state,
            msgs, count, info)
        n = ctypes.c_uint32()
        p = ctypes.c_void_p
        rc = self._L.wsg_reply_streams(self._ctx, p(wire.data_ptr()), wire.numel(), p(spans.data_ptr()), ns,
                                       p(state.data_ptr()), p(frame_start.data_ptr()), fcap,
                                       p(stream_first.data_ptr()), rule, 1 if mask else 0,
                                       p(send_keys.data_ptr()) if send_keys is not None else None,
                                       p(reply.data_ptr()), cap, p(reply_off.data_ptr()), p(stream_reply.data_ptr()),
                                       p(msgs.data_ptr()), p(count.data_ptr()), p(info.data_ptr()), ctypes.byref(n),
                                       self._stream(stream))
        _check(rc, "wsg_reply_streams")
        return reply, reply_off, stream_reply, msgs, count, state, info, frame_start, stream_first, n.value

    # -- checked replies (reply_messages with check_protocol inside it) --------
    def _checked_args(self, what, dev, ns, proto, close_off, verdict, result, count):
        t = self._torch
        if proto is None:
            proto = t.zeros(max(ns, 1) * PROTO_STATE.itemsize, dtype=t.uint8, device=dev)
        if close_off is None:
            close_off = t.empty(max(ns, 1), dtype=t.int64, device=dev)
        if verdict is None:
            verdict = t.empty(max(ns, 1) * PROTO_VERDICT.itemsize, dtype=t.uint8, device=dev)
        if result is None:
            result = t.empty(3, dtype=t.int64, device=dev)
        if count is None:
            count = t.empty(5, dtype=t.int64, device=dev)
        if (int(proto.numel()) * proto.element_size() < ns * PROTO_STATE.itemsize
                or int(close_off.numel()) < ns or close_off.element_size() != 8
                or int(verdict.numel()) * verdict.element_size() < ns * PROTO_VERDICT.itemsize
                or int(result.numel()) < 3 or result.element_size() != 8
                or int(count.numel()) < 5 or count.element_size() != 8):
            raise WSGError(WSG_EINVAL, "%s: a buffer is smaller than the batch needs" % what)
        return proto, close_off, verdict, result, count

    def reply_checked(self, wire, frame_start, stream_first, proto=None, role=PROTO_ANY, max_message=0, also=None,
                      reply_op=ECHO_REPLY, mask=False, send_keys=None, state=None, reply=None, reply_cap=None,
                      stream=None, reply_off=None, stream_reply=None, close_off=None, verdict=None, result=None,
                      msgs=None, count=None, info=None):
        """wsg_reply_checked: reply_messages with check_protocol run inside
        it.  Replies stop at a stream's terminal frame, where the stream gets
        a close frame with the verdict's status.  ``proto`` / ``role`` /
        ``max_message`` as check_protocol; ``also``: PROTO_VERDICT bytes per
        stream (utf8_verdicts' output) or None; the rest as reply_messages.
        Returns (reply, reply_off, stream_reply, close_off, verdict, proto,
        result, msgs, count, state, info): close_off int64[n_streams] (-1: no
        close frame), count int64[5] = [messages, dense bytes, reply bytes,
        reply frames, close frames]."""
        n = int(frame_start.numel())
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "reply_checked: stream_first must hold n_streams + 1 32-bit indices")
        proto, close_off, verdict, result, count = self._checked_args("reply_checked", wire.device, ns, proto,
                                                                      close_off, verdict, result, count)
        if also is not None and int(also.numel()) * also.element_size() < ns * PROTO_VERDICT.itemsize:
            raise WSGError(WSG_EINVAL, "reply_checked: also must hold n_streams verdicts")
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "reply_checked", wire, n, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply, state, msgs,
            count, info)
        p = ctypes.c_void_p
        rc = self._L.wsg_reply_checked(self._ctx, p(wire.data_ptr()), wire.numel(), p(frame_start.data_ptr()), n,
                                       p(stream_first.data_ptr()), ns, p(state.data_ptr()), p(proto.data_ptr()),
                                       int(role), int(max_message), p(also.data_ptr()) if also is not None else None,
                                       rule, 1 if mask else 0,
                                       p(send_keys.data_ptr()) if send_keys is not None else None,
                                       p(reply.data_ptr()), cap, p(reply_off.data_ptr()), p(stream_reply.data_ptr()),
                                       p(close_off.data_ptr()), p(verdict.data_ptr()), p(result.data_ptr()),
                                       p(msgs.data_ptr()), p(count.data_ptr()), p(info.data_ptr()),
                                       self._stream(stream))
        _check(rc, "wsg_reply_checked")
        return reply, reply_off, stream_reply, close_off, verdict, proto, result, msgs, count, state, info

    def reply_checked_streams(self, wire, spans, proto=None, role=PROTO_ANY, max_message=0, reply_op=ECHO_REPLY,
                              mask=False, send_keys=None, state=None, frame_start=None, frame_cap=None,
                              stream_first=None, reply=None, reply_cap=None, stream=None, reply_off=None,
                              stream_reply=None, close_off=None, verdict=None, result=None, msgs=None, count=None,
                              info=None):
        """wsg_reply_checked_streams: reply_streams with reply_checked in the
        middle.  Returns reply_checked's tuple followed by (frame_start,
        stream_first, n_frames)."""
        ns, fcap, frame_start, stream_first = self._frame_args("reply_checked_streams", wire, spans, frame_start,
                                                               frame_cap, stream_first)
        proto, close_off, verdict, result, count = self._checked_args("reply_checked_streams", wire.device, ns, proto,
                                                                      close_off, verdict, result, count)
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "reply_checked_streams", wire, fcap, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply,
            state, msgs, count, info)
        n = ctypes.c_uint32()
        p = ctypes.c_void_p
        rc = self._L.wsg_reply_checked_streams(
            self._ctx, p(wire.data_ptr()), wire.numel(), p(spans.data_ptr()), ns, p(state.data_ptr()),
            p(frame_start.data_ptr()), fcap, p(stream_first.data_ptr()), p(proto.data_ptr()), int(role),
            int(max_message), rule, 1 if mask else 0, p(send_keys.data_ptr()) if send_keys is not None else None,
            p(reply.data_ptr()), cap, p(reply_off.data_ptr()), p(stream_reply.data_ptr()), p(close_off.data_ptr()),
            p(verdict.data_ptr()), p(result.data_ptr()), p(msgs.data_ptr()), p(count.data_ptr()), p(info.data_ptr()),
            ctypes.byref(n), self._stream(stream))
        _check(rc, "wsg_reply_checked_streams")
        return (reply, reply_off, stream_reply, close_off, verdict, proto, result, msgs, count, state, info,
                frame_start, stream_first, n.value)

    # -- validated replies (reply_checked with check_utf8_wire inside it) -------
    def _validated_args(self, what, dev, n, valid, utf8_result):
        t = self._torch
        if valid is None:
            valid = t.empty(max(n, 1), dtype=t.int64, device=dev)
        if utf8_result is None:
            utf8_result = t.empty(4, dtype=t.int64, device=dev)
        if (int(valid.numel()) < n or valid.element_size() != 8 or int(utf8_result.numel()) < 4
                or utf8_result.element_size() != 8):
            raise WSGError(WSG_EINVAL, "%s: a buffer is smaller than the batch needs" % what)
        return valid, utf8_result

    def reply_validated(self, wire, frame_start, stream_first, proto=None, role=PROTO_ANY, max_message=0, also=None,
                        which=UTF8_TEXT | UTF8_CLOSE, reply_op=ECHO_REPLY, mask=False, send_keys=None, state=None,
                        reply=None, reply_cap=None, stream=None, reply_off=None, stream_reply=None, close_off=None,
                        verdict=None, result=None, valid=None, utf8_result=None, msgs=None, count=None, info=None):
        """wsg_reply_validated: reply_checked with the UTF-8 check of
        check_utf8_wire inside it; a stream whose text message or close
        reason is invalid gets the 1007 close frame at that message's FIN
        frame.  Arguments as reply_checked, and ``which`` (UTF8_* bits).
        Returns reply_checked's tuple followed by (valid, utf8_result) as
        check_utf8_wire returns them."""
        n = int(frame_start.numel())
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "reply_validated: stream_first must hold n_streams + 1 32-bit indices")
        proto, close_off, verdict, result, count = self._checked_args("reply_validated", wire.device, ns, proto,
                                                                      close_off, verdict, result, count)
        if also is not None and int(also.numel()) * also.element_size() < ns * PROTO_VERDICT.itemsize:
            raise WSGError(WSG_EINVAL, "reply_validated: also must hold n_streams verdicts")
        valid, utf8_result = self._validated_args("reply_validated", wire.device, n, valid, utf8_result)
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "reply_validated", wire, n, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply, state,
            msgs, count, info)
        p = ctypes.c_void_p
        rc = self._L.wsg_reply_validated(self._ctx, p(wire.data_ptr()), wire.numel(), p(frame_start.data_ptr()), n,
                                         p(stream_first.data_ptr()), ns, p(state.data_ptr()), p(proto.data_ptr()),
                                         int(role), int(max_message), p(also.data_ptr()) if also is not None else None,
                                         int(which), rule, 1 if mask else 0,
                                         p(send_keys.data_ptr()) if send_keys is not None else None,
                                         p(reply.data_ptr()), cap, p(reply_off.data_ptr()),
                                         p(stream_reply.data_ptr()), p(close_off.data_ptr()), p(verdict.data_ptr()),
                                         p(result.data_ptr()), p(valid.data_ptr()), p(utf8_result.data_ptr()),
                                         p(msgs.data_ptr()), p(count.data_ptr()), p(info.data_ptr()),
                                         self._stream(stream))
        _check(rc, "wsg_reply_validated")
        return (reply, reply_off, stream_reply, close_off, verdict, proto, result, msgs, count, state, info, valid,
                utf8_result)

    def reply_validated_streams(self, wire, spans, proto=None, role=PROTO_ANY, max_message=0,
                                which=UTF8_TEXT | UTF8_CLOSE, reply_op=ECHO_REPLY, mask=False, send_keys=None,
                                state=None, frame_start=None, frame_cap=None, stream_first=None, reply=None,
                                reply_cap=None, stream=None, reply_off=None, stream_reply=None, close_off=None,
                                verdict=None, result=None, valid=None, utf8_result=None, msgs=None, count=None,
                                info=None):
        """wsg_reply_validated_streams: reply_checked_streams with
        reply_validated in the middle.  Returns reply_validated's tuple
        followed by (frame_start, stream_first, n_frames)."""
        ns, fcap, frame_start, stream_first = self._frame_args("reply_validated_streams", wire, spans, frame_start,
                                                               frame_cap, stream_first)
        proto, close_off, verdict, result, count = self._checked_args("reply_validated_streams", wire.device, ns,
                                                                      proto, close_off, verdict, result, count)
        valid, utf8_result = self._validated_args("reply_validated_streams", wire.device, fcap, valid, utf8_result)
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "reply_validated_streams", wire, fcap, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply,
            state, msgs, count, info)
        n = ctypes.c_uint32()
        p = ctypes.c_void_p
        rc = self._L.wsg_reply_validated_streams(
            self._ctx, p(wire.data_ptr()), wire.numel(), p(spans.data_ptr()), ns, p(state.data_ptr()),
            p(frame_start.data_ptr()), fcap, p(stream_first.data_ptr()), p(proto.data_ptr()), int(role),
            int(max_message), int(which), rule, 1 if mask else 0,
            p(send_keys.data_ptr()) if send_keys is not None else None, p(reply.data_ptr()), cap,
            p(reply_off.data_ptr()), p(stream_reply.data_ptr()), p(close_off.data_ptr()), p(verdict.data_ptr()),
            p(result.data_ptr()), p(valid.data_ptr()), p(utf8_result.data_ptr()), p(msgs.data_ptr()),
            p(count.data_ptr()), p(info.data_ptr()), ctypes.byref(n), self._stream(stream))
        _check(rc, "wsg_reply_validated_streams")
        return (reply, reply_off, stream_reply, close_off, verdict, proto, result, msgs, count, state, info, valid,
                utf8_result, frame_start, stream_first, n.value)

    # -- relays (reply_validated with a chat server's rooms behind it) -----------
    def _relay_args(self, what, wire, n, ns, relay_op, order, group_first, relay, relay_cap, relay_off, group_relay,
                    count):
        t = self._torch
        dev = wire.device
        rule = bytes(int(x) for x in relay_op)
        if len(rule) != 5:
            raise WSGError(WSG_EINVAL, "%s: relay_op must hold five bytes (indexed by CB_*)" % what)
        if order is not None and (order.element_size() != 4 or int(order.numel()) < ns):
            raise WSGError(WSG_EINVAL, "%s: order must hold n_streams 32-bit indices" % what)
        if group_first is not None and (group_first.element_size() != 4 or int(group_first.numel()) < 1):
            raise WSGError(WSG_EINVAL, "%s: group_first must hold n_groups + 1 32-bit positions" % what)
        ng = int(group_first.numel()) - 1 if group_first is not None else 1
        if relay_cap is None:   # as reply_cap: wire bytes + 14 * n always suffices
            relay_cap = int(wire.numel()) + 14 * n if relay is None else int(relay.numel())
        cap = int(relay_cap)
        if relay is None:
            relay = t.empty(max(cap, 16), dtype=t.uint8, device=dev)
        if relay_off is None:
            relay_off = t.empty(max(n, 1), dtype=t.int64, device=dev)
        if group_relay is None:
            group_relay = t.empty(ng + 1, dtype=t.int64, device=dev)
        if count is None:
            count = t.empty(8, dtype=t.int64, device=dev)
        if (cap > int(relay.numel()) or int(relay_off.numel()) < n or relay_off.element_size() != 8
                or int(group_relay.numel()) < ng + 1 or group_relay.element_size() != 8
                or int(count.numel()) < 8 or count.element_size() != 8):
            raise WSGError(WSG_EINVAL, "%s: a buffer is smaller than the batch needs" % what)
        return rule, ng, cap, relay, relay_off, group_relay, count

    def relay_validated(self, wire, frame_start, stream_first, proto=None, role=PROTO_ANY, max_message=0, also=None,
                        which=UTF8_TEXT | UTF8_CLOSE, reply_op=CHAT_REPLY, mask=False, send_keys=None,
                        relay_op=CHAT_RELAY, order=None, group_first=None, state=None, reply=None, reply_cap=None,
                        relay=None, relay_cap=None, stream=None, reply_off=None, stream_reply=None, close_off=None,
                        relay_off=None, group_relay=None, verdict=None, result=None, valid=None, utf8_result=None,
                        msgs=None, count=None, info=None):
        """wsg_relay_validated: reply_validated, and the messages whose kind
        ``relay_op`` names (five bytes by CB_*, as reply_op; a kind is replied
        to or relayed, not both) written once as unmasked server frames into
        ``relay``, one range per room.  ``order``: int32 CUDA tensor, a
        permutation of the stream indices (None: the identity);
        ``group_first``: int32 CUDA tensor of n_groups + 1 positions (None: one
        room of everyone).  Returns reply_validated's tuple, its count int64[8]
        = [.., relay bytes, relay frames, 0], followed by (relay, relay_off,
        group_relay): int64[n] frame starts per message (-1: not relayed;
        count[0] valid) and int64[n_groups + 1] offsets per room.
        ``relay_cap`` defaults to wire bytes + 14 * n, which always suffices."""
        n = int(frame_start.numel())
        ns = int(stream_first.numel()) - 1
        if ns < 0 or stream_first.element_size() != 4:
            raise WSGError(WSG_EINVAL, "relay_validated: stream_first must hold n_streams + 1 32-bit indices")
        rrule, ng, rcap, relay, relay_off, group_relay, count = self._relay_args(
            "relay_validated", wire, n, ns, relay_op, order, group_first, relay, relay_cap, relay_off, group_relay,
            count)
        proto, close_off, verdict, result, count = self._checked_args("relay_validated", wire.device, ns, proto,
                                                                      close_off, verdict, result, count)
        if also is not None and int(also.numel()) * also.element_size() < ns * PROTO_VERDICT.itemsize:
            raise WSGError(WSG_EINVAL, "relay_validated: also must hold n_streams verdicts")
        valid, utf8_result = self._validated_args("relay_validated", wire.device, n, valid, utf8_result)
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "relay_validated", wire, n, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply, state,
            msgs, count, info)
        p = ctypes.c_void_p
        rc = self._L.wsg_relay_validated(
            self._ctx, p(wire.data_ptr()), wire.numel(), p(frame_start.data_ptr()), n, p(stream_first.data_ptr()), ns,
            p(state.data_ptr()), p(proto.data_ptr()), int(role), int(max_message),
            p(also.data_ptr()) if also is not None else None, int(which), rule, 1 if mask else 0,
            p(send_keys.data_ptr()) if send_keys is not None else None, rrule,
            p(order.data_ptr()) if order is not None else None,
            p(group_first.data_ptr()) if group_first is not None else None, ng, p(reply.data_ptr()), cap,
            p(reply_off.data_ptr()), p(stream_reply.data_ptr()), p(close_off.data_ptr()), p(relay.data_ptr()), rcap,
            p(relay_off.data_ptr()), p(group_relay.data_ptr()), p(verdict.data_ptr()), p(result.data_ptr()),
            p(valid.data_ptr()), p(utf8_result.data_ptr()), p(msgs.data_ptr()), p(count.data_ptr()),
            p(info.data_ptr()), self._stream(stream))
        _check(rc, "wsg_relay_validated")
        return (reply, reply_off, stream_reply, close_off, verdict, proto, result, msgs, count, state, info, valid,
                utf8_result, relay, relay_off, group_relay)

    def relay_validated_streams(self, wire, spans, proto=None, role=PROTO_ANY, max_message=0,
                                which=UTF8_TEXT | UTF8_CLOSE, reply_op=CHAT_REPLY, mask=False, send_keys=None,
                                relay_op=CHAT_RELAY, order=None, group_first=None, state=None, frame_start=None,
                                frame_cap=None, stream_first=None, reply=None, reply_cap=None, relay=None,
                                relay_cap=None, stream=None, reply_off=None, stream_reply=None, close_off=None,
                                relay_off=None, group_relay=None, verdict=None, result=None, valid=None,
                                utf8_result=None, msgs=None, count=None, info=None):
        """wsg_relay_validated_streams: reply_validated_streams with
        relay_validated in the middle.  Returns relay_validated's tuple
        followed by (frame_start, stream_first, n_frames)."""
        ns, fcap, frame_start, stream_first = self._frame_args("relay_validated_streams", wire, spans, frame_start,
                                                               frame_cap, stream_first)
        rrule, ng, rcap, relay, relay_off, group_relay, count = self._relay_args(
            "relay_validated_streams", wire, fcap, ns, relay_op, order, group_first, relay, relay_cap, relay_off,
            group_relay, count)
        proto, close_off, verdict, result, count = self._checked_args("relay_validated_streams", wire.device, ns,
                                                                      proto, close_off, verdict, result, count)
        valid, utf8_result = self._validated_args("relay_validated_streams", wire.device, fcap, valid, utf8_result)
        rule, cap, reply, reply_off, stream_reply, state, msgs, count, info = self._reply_args(
            "relay_validated_streams", wire, fcap, ns, reply_op, send_keys, reply, reply_cap, reply_off, stream_reply,
            state, msgs, count, info)
        n = ctypes.c_uint32()
        p = ctypes.c_void_p
        rc = self._L.wsg_relay_validated_streams(
            self._ctx, p(wire.data_ptr()), wire.numel(), p(spans.data_ptr()), ns, p(state.data_ptr()),
            p(frame_start.data_ptr()), fcap, p(stream_first.data_ptr()), p(proto.data_ptr()), int(role),
            int(max_message), int(which), rule, 1 if mask else 0,
            p(send_keys.data_ptr()) if send_keys is not None else None, rrule,
            p(order.data_ptr()) if order is not None else None,
            p(group_first.data_ptr()) if group_first is not None else None, ng, p(reply.data_ptr()), cap,
            p(reply_off.data_ptr()), p(stream_reply.data_ptr()), p(close_off.data_ptr()), p(relay.data_ptr()), rcap,
            p(relay_off.data_ptr()), p(group_relay.data_ptr()), p(verdict.data_ptr()), p(result.data_ptr()),
            p(valid.data_ptr()), p(utf8_result.data_ptr()), p(msgs.data_ptr()), p(count.data_ptr()),
            p(info.data_ptr()), ctypes.byref(n), self._stream(stream))
        _check(rc, "wsg_relay_validated_streams")
        return (reply, reply_off, stream_reply, close_off, verdict, proto, result, msgs, count, state, info, valid,
                utf8_result, relay, relay_off, group_relay, frame_start, stream_first, n.value)

    def utf8_verdicts(self, msgs, count, valid, n_streams, which=UTF8_TEXT | UTF8_CLOSE, msg_room=None, also=None,
                      stream=None):
        """wsg_utf8_verdicts: check_utf8's ``valid`` as reply_checked's
        ``also``: PROTO_VERDICT bytes per stream, all 0xFF or {PV_UTF8, 1007,
        the FIN frame of the stream's first invalid message}.  ``which`` as
        given to check_utf8."""
        t = self._torch
        ns = int(n_streams)
        if msg_room is None:
            msg_room = min(int(msgs.numel()) // MSG.itemsize, int(valid.numel()))
        room = int(msg_room)
        if also is None:
            also = t.empty(max(ns, 1) * PROTO_VERDICT.itemsize, dtype=t.uint8, device=msgs.device)
        if (int(msgs.numel()) < room * MSG.itemsize or int(valid.numel()) < room or valid.element_size() != 8
                or int(count.numel()) < 2 or count.element_size() != 8
                or int(also.numel()) * also.element_size() < ns * PROTO_VERDICT.itemsize):
            raise WSGError(WSG_EINVAL, "utf8_verdicts: a buffer is smaller than the batch needs")
        p = ctypes.c_void_p
        rc = self._L.wsg_utf8_verdicts(self._ctx, p(msgs.data_ptr()), p(count.data_ptr()), room, int(which),
                                       p(valid.data_ptr()), ns, p(also.data_ptr()), self._stream(stream))
        _check(rc, "wsg_utf8_verdicts")
        return also

    def prepare_decode(self, wire, frame_start, out, info, stream=None):
        """wsg_decode_batch on fixed buffers (a server's batch arena), with
        the ctypes arguments bound once: returns a callable that launches one
        decode per call (asynchronous, like decode_batch)."""
        n = int(frame_start.numel())
        if int(out.numel()) < int(wire.numel()) or int(info.numel()) < n * RECV_INFO.itemsize:
            raise WSGError(WSG_EINVAL, "prepare_decode: out or info smaller than the batch needs")
        fn = self._L.wsg_decode_batch
        args = (self._ctx, ctypes.c_void_p(wire.data_ptr()), ctypes.c_uint64(wire.numel()),
                ctypes.c_void_p(frame_start.data_ptr()), ctypes.c_uint32(n), ctypes.c_void_p(out.data_ptr()),
                ctypes.c_void_p(info.data_ptr()))
        keep = (wire, frame_start, out, info)   # the buffers live as long as the callable
        fixed = None if stream is None else self._stream(stream)

        def launch():
            # stream=None: torch's current stream at each launch, as decode_batch
            rc = fn(*args, fixed if fixed is not None else self._stream(None))
            if rc != 0:
                raise WSGError(rc, "wsg_decode_batch")
            return keep

        return launch

    def prepare_fanout(self, payload, keys, opcode, mask, wire, length=None, stream=None):
        """wsg_fanout_encode on fixed buffers with the ctypes arguments bound
        once (the multicast loop of a server); returns a launch callable."""
        k = int(keys.numel())
        length = int(payload.numel()) if length is None else int(length)
        if frame_size(opcode, mask, length) * k > int(wire.numel()):
            raise WSGError(WSG_ENOMEM, "prepare_fanout: wire smaller than %d frames" % k)
        fn = self._L.wsg_fanout_encode
        args = (self._ctx, ctypes.c_void_p(payload.data_ptr()), ctypes.c_uint64(length),
                ctypes.c_void_p(keys.data_ptr()), ctypes.c_uint32(k), ctypes.c_uint8(opcode), 1 if mask else 0,
                ctypes.c_void_p(wire.data_ptr()), ctypes.c_uint64(wire.numel()))
        keep = (payload, keys, wire)
        fixed = None if stream is None else self._stream(stream)

        def launch():
            # stream=None: torch's current stream at each launch, as fanout
            rc = fn(*args, fixed if fixed is not None else self._stream(None))
            if rc != 0:
                raise WSGError(rc, "wsg_fanout_encode")
            return keep

        return launch

    # -- batch encode (mask) --------------------------------------------------
    def encode_batch(self, payload, desc, wire=None, wire_cap=None, wire_off=None, stream=None):
        """Encode frames ``desc`` (uint8 CUDA tensor of n*32 bytes) whose data
        live in ``payload``.  Returns (wire, wire_off int64[n+1])."""
        t = self._torch
        n = int(desc.numel() // SEND_DESC.itemsize)
        if wire is None:
            wire = t.empty(max(int(wire_cap), 16), dtype=t.uint8, device=desc.device)
        cap = int(wire.numel()) if wire_cap is None else int(wire_cap)
        if cap > int(wire.numel()):
            raise WSGError(WSG_EINVAL, "encode_batch: wire_cap %d exceeds the wire tensor (%d bytes)"
                           % (cap, int(wire.numel())))
        if wire_off is None:
            wire_off = t.empty(n + 1, dtype=t.int64, device=desc.device)
        rc = self._L.wsg_encode_batch(self._ctx, ctypes.c_void_p(payload.data_ptr()),
                                      ctypes.c_void_p(desc.data_ptr()), n, ctypes.c_void_p(wire.data_ptr()),
                                      cap, ctypes.c_void_p(wire_off.data_ptr()), self._stream(stream))
        _check(rc, "wsg_encode_batch")
        return wire, wire_off

    def fanout(self, payload, keys, opcode, mask=True, wire=None, length=None, stream=None):
        t = self._torch
        k = int(keys.numel())
        length = int(payload.numel()) if length is None else int(length)
        fsz = frame_size(opcode, mask, length)
        if wire is None:
            wire = t.empty(max(fsz * k, 16), dtype=t.uint8, device=payload.device)
        rc = self._L.wsg_fanout_encode(self._ctx, ctypes.c_void_p(payload.data_ptr()), length,
                                       ctypes.c_void_p(keys.data_ptr()), k, opcode, 1 if mask else 0,
                                       ctypes.c_void_p(wire.data_ptr()), wire.numel(), self._stream(stream))
        _check(rc, "wsg_fanout_encode")
        return wire

    def fanout_many(self, payload, src_off, lens, opcodes, keys, mask=True, wire=None, stream=None):
        """m messages (payload[src_off[i]:][:lens[i]], opcode opcodes[i]) x k
        keys in one call (wsg_fanout_encode_many).  Returns (wire, wire_off):
        message i's k frames start at wire_off[i] (host numpy, m + 1)."""
        t = self._torch
        src_off = np.ascontiguousarray(src_off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        opcodes = np.ascontiguousarray(opcodes, dtype=np.uint8)
        m, k = len(lens), int(keys.numel())
        need = 0
        for i in range(m):
            need = (need + 127) // 128 * 128 + frame_size(int(opcodes[i]), mask, int(lens[i])) * k
        if wire is None:
            wire = t.empty(max(need, 16), dtype=t.uint8, device=keys.device)
        off = np.zeros(m + 1, dtype=np.uint64)
        rc = self._L.wsg_fanout_encode_many(self._ctx, ctypes.c_void_p(payload.data_ptr()), _np_ptr(src_off),
                                            _np_ptr(lens), _np_ptr(opcodes), m, ctypes.c_void_p(keys.data_ptr()), k,
                                            1 if mask else 0, ctypes.c_void_p(wire.data_ptr()), wire.numel(),
                                            _np_ptr(off), self._stream(stream))
        _check(rc, "wsg_fanout_encode_many")
        return wire, off

    # -- host-staged paths ----------------------------------------------------
    def xor_host(self, data, key, phase=0):
        src = bytes(data)
        dst = ctypes.create_string_buffer(max(len(src), 1))
        _check(self._L.wsg_xor_host(self._ctx, src, dst, len(src), key, phase), "wsg_xor_host")
        return dst.raw[: len(src)]

    def decode_batch_host(self, wire, frame_start, out=None):
        wire = np.ascontiguousarray(wire, dtype=np.uint8)
        fs = np.ascontiguousarray(frame_start, dtype=np.uint64)
        if out is None:
            out = np.empty(max(len(wire), 1), dtype=np.uint8)
        info = np.zeros(max(len(fs), 1), dtype=RECV_INFO)
        rc = self._L.wsg_decode_batch_host(self._ctx, _np_ptr(wire), len(wire), _np_ptr(fs), len(fs),
                                           _np_ptr(out), _np_ptr(info))
        return rc, out[: len(wire)], info[: len(fs)]

    def encode_batch_host(self, payload, desc, wire=None):
        """Host-staged batch encode: returns (rc, wire bytes, wire_off)."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=SEND_DESC)
        n = len(desc)
        total = int(frame_sizes(desc).sum()) if n else 0
        if wire is None:
            wire = np.empty(max(total, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._L.wsg_encode_batch_host(self._ctx, _np_ptr(payload) if len(payload) else None, len(payload),
                                           _np_ptr(desc) if n else None, n, _np_ptr(wire), len(wire), _np_ptr(off))
        return rc, wire[:total], off

    # -- measurement hooks ----------------------------------------------------
    def timing(self, on=True, every=1):
        """Time the dominant kernel of every `every`-th batch call (HIP events)."""
        _check(self._L.wsg_timing_enable(self._ctx, int(every) if on else 0), "wsg_timing_enable")

    def timing_minmax(self):
        """(shortest, longest) timed launch in ms since the last reset."""
        lo, hi = ctypes.c_double(), ctypes.c_double()
        _check(self._L.wsg_timing_minmax(self._ctx, ctypes.byref(lo), ctypes.byref(hi)), "wsg_timing_minmax")
        return lo.value, hi.value

    def lane_stats(self):
        """(requests this context put on the lane, launches of the device's
        lane, running: 1 / 0 / -1 given up) — wsg_lane_stats."""
        r, l, on = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        _check(self._L.wsg_lane_stats(self._ctx, ctypes.byref(r), ctypes.byref(l), ctypes.byref(on)),
               "wsg_lane_stats")
        return r.value, l.value, on.value

    def lane_events(self):
        """(give-ups, re-arms) of the device's lane — wsg_lane_events."""
        g, r = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.wsg_lane_events(self._ctx, ctypes.byref(g), ctypes.byref(r)), "wsg_lane_events")
        return g.value, r.value

    def timing_read(self, reset=True):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        _check(self._L.wsg_timing_read(self._ctx, ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0),
               "wsg_timing_read")
        return ms.value, n.value


RECEIVE_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
                              ctypes.c_int)
RX_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8),
                         ctypes.c_size_t, ctypes.c_int)


class Session:
    """One connection's codec state through the C-ABI (wsg_session_*): the
    reference WebSocket mix-in with its payload XOR on the GPU."""

    def __init__(self, codec, send_key=0):
        self._L = lib()
        self._codec = codec          # keeps the ctx alive
        s = ctypes.c_void_p()
        _check(self._L.wsg_session_create(codec._ctx, ctypes.byref(s)), "wsg_session_create")
        self._s = s
        self.set_send_key(send_key)
        self._events = []

        def _cb(user, kind, data, size, status):
            self._events.append((kind, ctypes.string_at(data, size) if size else b"", status))

        self._cb = RECEIVE_CB(_cb)

    def close(self):
        if getattr(self, "_s", None):
            self._L.wsg_session_destroy(self._s)
            self._s = None

    __del__ = close

    def set_send_key(self, key):
        _check(self._L.wsg_session_set_send_key(self._s, key), "wsg_session_set_send_key")

    def prepare_send(self, opcode, mask, payload=b"", status=0):
        buf = bytes(payload)
        cap = frame_size(opcode, mask, len(buf), status)
        out = ctypes.create_string_buffer(max(cap, 1))
        n = ctypes.c_size_t()
        _check(self._L.wsg_session_prepare_send(self._s, opcode, 1 if mask else 0, buf, len(buf), status, out, cap,
                                                ctypes.byref(n)), "wsg_session_prepare_send")
        return out.raw[: n.value]

    def prepare_receive(self, data):
        buf = bytes(data)
        _check(self._L.wsg_session_prepare_receive(self._s, buf if buf else None, len(buf), self._cb, None),
               "wsg_session_prepare_receive")

    def events(self, clear=True):
        ev = list(self._events)
        if clear:
            self._events.clear()
        return ev

    def required(self):
        return self._L.wsg_session_required(self._s)

    def clear(self):
        _check(self._L.wsg_session_clear(self._s), "wsg_session_clear")


class RxBatch:
    """Batched receive over many sessions through the C-ABI (wsg_rx_*): feed()
    frames each session's stream on the host, flush() unmasks the batch in one
    GPU pass and fires every session's callbacks in arrival order.  Events are
    (session, kind, payload bytes, status)."""

    def __init__(self, codec):
        self._L = lib()
        self._codec = codec
        rx = ctypes.c_void_p()
        _check(self._L.wsg_rx_create(codec._ctx, ctypes.byref(rx)), "wsg_rx_create")
        self._rx = rx
        self._events = []
        self._by_ptr = {}

        def _cb(user, sess, kind, data, size, status):
            self._events.append((self._by_ptr.get(sess), kind, ctypes.string_at(data, size) if size else b"",
                                 status))

        self._cb = RX_CB(_cb)

    def close(self):
        if getattr(self, "_rx", None):
            self._L.wsg_rx_destroy(self._rx)
            self._rx = None

    __del__ = close

    def _reg(self, session):
        self._by_ptr[session._s.value] = session
        return session._s

    def feed(self, session, data):
        buf = bytes(data)
        _check(self._L.wsg_rx_feed(self._rx, self._reg(session), buf if buf else None, len(buf)), "wsg_rx_feed")

    def clear(self, session):
        _check(self._L.wsg_rx_clear(self._rx, self._reg(session)), "wsg_rx_clear")

    def forget(self, session):
        _check(self._L.wsg_rx_forget(self._rx, self._reg(session)), "wsg_rx_forget")

    def pending(self):
        f, b = ctypes.c_uint32(), ctypes.c_uint64()
        _check(self._L.wsg_rx_pending(self._rx, ctypes.byref(f), ctypes.byref(b)), "wsg_rx_pending")
        return f.value, b.value

    def set_devices(self, devices):
        """Spread every flush over these GPUs (wsg_rx_set_devices)."""
        d = (ctypes.c_int * max(len(devices), 1))(*devices)
        _check(self._L.wsg_rx_set_devices(self._rx, d, len(devices)), "wsg_rx_set_devices")

    def flush(self):
        n = ctypes.c_uint32()
        _check(self._L.wsg_rx_flush(self._rx, self._cb, None, ctypes.byref(n)), "wsg_rx_flush")
        return n.value

    def events(self, clear=True):
        ev = list(self._events)
        if clear:
            self._events.clear()
        return ev


TX_SINK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t)


class TxBatch:
    """Batched send over many sessions through the C-ABI (wsg_tx_*): queue()
    records a PrepareSendFrame call, flush() encodes all of them in one GPU
    pass and returns [(session, frame bytes)] in queue order."""

    def __init__(self, codec):
        self._L = lib()
        self._codec = codec
        tx = ctypes.c_void_p()
        _check(self._L.wsg_tx_create(codec._ctx, ctypes.byref(tx)), "wsg_tx_create")
        self._tx = tx
        self._out = []
        self._by_ptr = {}

        def _sink(user, sess, frame, size):
            self._out.append((self._by_ptr.get(sess), ctypes.string_at(frame, size)))

        self._sink = TX_SINK(_sink)

    def close(self):
        if getattr(self, "_tx", None):
            self._L.wsg_tx_destroy(self._tx)
            self._tx = None

    __del__ = close

    def queue(self, session, opcode, mask, payload=b"", status=0):
        self._by_ptr[session._s.value] = session
        buf = bytes(payload)
        _check(self._L.wsg_tx_queue(self._tx, session._s, opcode, 1 if mask else 0, buf if buf else None, len(buf),
                                    status), "wsg_tx_queue")

    def forget(self, session):
        _check(self._L.wsg_tx_forget(self._tx, session._s), "wsg_tx_forget")

    def pending(self):
        f, b = ctypes.c_uint32(), ctypes.c_uint64()
        _check(self._L.wsg_tx_pending(self._tx, ctypes.byref(f), ctypes.byref(b)), "wsg_tx_pending")
        return f.value, b.value

    def set_devices(self, devices):
        """Spread every flush over these GPUs (wsg_tx_set_devices)."""
        d = (ctypes.c_int * max(len(devices), 1))(*devices)
        _check(self._L.wsg_tx_set_devices(self._tx, d, len(devices)), "wsg_tx_set_devices")

    def flush(self):
        n = ctypes.c_uint32()
        self._out = []
        _check(self._L.wsg_tx_flush(self._tx, self._sink, None, ctypes.byref(n)), "wsg_tx_flush")
        out, self._out = self._out, []
        if len(out) != n.value:
            raise WSGError(WSG_EINVAL, "wsg_tx_flush: %d frames handed out, %d reported" % (len(out), n.value))
        return out


def info_to_numpy(info_tensor, n):
    """Device info bytes -> numpy RECV_INFO records."""
    return info_tensor[: n * RECV_INFO.itemsize].cpu().numpy().view(RECV_INFO)


def desc_to_tensor(desc, device):
    import torch

    desc = np.ascontiguousarray(desc, dtype=SEND_DESC)
    return torch.from_numpy(desc.view(np.uint8).copy()).to(device)


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[ctypes.c_void_p(p) for p in ptrs])


def _host_decode_args(wire, frame_start, out):
    wire = np.ascontiguousarray(wire, dtype=np.uint8)
    fs = np.ascontiguousarray(frame_start, dtype=np.uint64)
    if out is None:
        out = np.empty(max(len(wire), 1), dtype=np.uint8)
    info = np.zeros(max(len(fs), 1), dtype=RECV_INFO)
    return wire, fs, out, info


def _host_encode_args(payload, desc, wire):
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    desc = np.ascontiguousarray(desc, dtype=SEND_DESC)
    total = int(frame_sizes(desc).sum()) if len(desc) else 0
    if wire is None:
        wire = np.empty(max(total, 1), dtype=np.uint8)
    off = np.zeros(len(desc) + 1, dtype=np.uint64)
    return payload, desc, wire, off, total


def decode_batch_host_multi(codecs, wire, frame_start, out=None):
    """wsg_decode_batch_host_multi: one host batch over several contexts
    (their GPUs' PCIe links at once).  Returns (rc, out, info) like
    Codec.decode_batch_host."""
    wire, fs, out, info = _host_decode_args(wire, frame_start, out)
    ctxs = _ptr_array([c._ctx.value for c in codecs])
    rc = lib().wsg_decode_batch_host_multi(ctxs, len(codecs), _np_ptr(wire), len(wire), _np_ptr(fs), len(fs),
                                           _np_ptr(out), _np_ptr(info))
    return rc, out[: len(wire)], info[: len(fs)]


def encode_batch_host_multi(codecs, payload, desc, wire=None):
    """wsg_encode_batch_host_multi: returns (rc, wire bytes, wire_off)."""
    payload, desc, wire, off, total = _host_encode_args(payload, desc, wire)
    ctxs = _ptr_array([c._ctx.value for c in codecs])
    n = len(desc)
    rc = lib().wsg_encode_batch_host_multi(ctxs, len(codecs), _np_ptr(payload) if len(payload) else None,
                                           len(payload), _np_ptr(desc) if n else None, n, _np_ptr(wire), len(wire),
                                           _np_ptr(off))
    return rc, wire[:total], off


class MultiGPU:
    """The multi-GPU entry of the C-ABI (wsg_mgpu_*): round-robin shards of a
    frame batch encoded on their GPUs and gathered to one rank.

    MultiGPU(devices=[0, 1, ...]) drives every rank from this process, one
    rank per listed device (a device may be listed more than once): chunks
    move to the root by device copies (xGMI peer copies between GPUs);
    MultiGPU.rank(device, uid, rank, world) is one rank of a multi-process
    group over RCCL (uid from MultiGPU.unique_id() on rank 0, handed to
    every rank)."""

    ID_BYTES = 128

    def __init__(self, devices=None, _handle=None):
        self._L = lib()
        if _handle is not None:
            self._g = _handle
        else:
            devs = (ctypes.c_int * len(devices))(*devices)
            g = ctypes.c_void_p()
            _check(self._L.wsg_mgpu_create(devs, len(devices), ctypes.byref(g)), "wsg_mgpu_create")
            self._g = g
        w, nl, fr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self._L.wsg_mgpu_info(self._g, ctypes.byref(w), ctypes.byref(nl), ctypes.byref(fr)), "wsg_mgpu_info")
        self.world, self.nlocal, self.first_rank = w.value, nl.value, fr.value

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * MultiGPU.ID_BYTES)()
        _check(lib().wsg_mgpu_unique_id(buf), "wsg_mgpu_unique_id")
        return bytes(buf)

    @classmethod
    def rank(cls, device, uid, rank, world):
        g = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * cls.ID_BYTES).from_buffer_copy(bytes(uid))
        _check(lib().wsg_mgpu_create_rank(device, buf, rank, world, ctypes.byref(g)), "wsg_mgpu_create_rank")
        return cls(_handle=g)

    @staticmethod
    def shard_count(n_total, chunk, world, rank):
        return int(lib().wsg_mgpu_shard_count(n_total, chunk, world, rank))

    def close(self):
        if getattr(self, "_g", None):
            self._L.wsg_mgpu_destroy(self._g)
            self._g = None

    __del__ = close

    def _ctx(self, i):
        ctx = self._L.wsg_mgpu_ctx(self._g, int(i))
        if not ctx:
            raise WSGError(WSG_EINVAL, "wsg_mgpu_ctx(%d)" % i)
        return ctypes.c_void_p(ctx)

    def timing(self, on=True, every=1, i=0):
        """Time the dominant kernel of local rank i's encodes (its context's
        HIP events, as Codec.timing): k_encode_mask inside encode_gather."""
        _check(self._L.wsg_timing_enable(self._ctx(i), int(every) if on else 0), "wsg_timing_enable")

    def timing_read(self, reset=True, i=0):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        _check(self._L.wsg_timing_read(self._ctx(i), ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0),
               "wsg_timing_read")
        return ms.value, n.value

    def encode_gather(self, n_total, chunk, payloads, descs, wires, wire_offs, root=0, out=None, out_off=None):
        """Per local rank (lists of CUDA tensors): payload arena, descriptor
        bytes (n_local * 32), wire buffer, wire_off (n_local + 1 int64).  On
        the root: `out` (uint8) and `out_off` (int64, n_total + 1, or None).
        Returns (encode_ms, gather_ms)."""
        k = self.nlocal
        n_local = (ctypes.c_uint32 * k)(*[int(d.numel()) // SEND_DESC.itemsize for d in descs])
        caps = (ctypes.c_uint64 * k)(*[int(w.numel()) for w in wires])
        times = (ctypes.c_double * 2)()
        rc = self._L.wsg_mgpu_encode_gather(
            self._g, int(n_total), int(chunk), _ptr_array([p.data_ptr() for p in payloads]),
            _ptr_array([d.data_ptr() for d in descs]), n_local, _ptr_array([w.data_ptr() for w in wires]), caps,
            _ptr_array([o.data_ptr() for o in wire_offs]), int(root),
            ctypes.c_void_p(out.data_ptr() if out is not None else 0), int(out.numel()) if out is not None else 0,
            ctypes.c_void_p(out_off.data_ptr() if out_off is not None else 0), times)
        _check(rc, "wsg_mgpu_encode_gather")
        return times[0], times[1]

    def decode_batch_host(self, wire, frame_start, out=None):
        """wsg_mgpu_decode_batch_host: a host batch over this process's GPUs."""
        wire, fs, out, info = _host_decode_args(wire, frame_start, out)
        rc = self._L.wsg_mgpu_decode_batch_host(self._g, _np_ptr(wire), len(wire), _np_ptr(fs), len(fs),
                                                _np_ptr(out), _np_ptr(info))
        return rc, out[: len(wire)], info[: len(fs)]

    def encode_batch_host(self, payload, desc, wire=None):
        payload, desc, wire, off, total = _host_encode_args(payload, desc, wire)
        n = len(desc)
        rc = self._L.wsg_mgpu_encode_batch_host(self._g, _np_ptr(payload) if len(payload) else None, len(payload),
                                                _np_ptr(desc) if n else None, n, _np_ptr(wire), len(wire),
                                                _np_ptr(off))
        return rc, wire[:total], off

