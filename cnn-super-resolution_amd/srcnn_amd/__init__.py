"""srcnn_amd -- Python binding of libsrcnn_hip.so over its C ABI (include/srcnn.h).

This is a thin ctypes layer: every call goes straight to an extern "C" entry
point of the HIP library; there is no Python or CPU implementation of any
operator behind it.  If the library is missing, importing this module fails
loudly (build it with `make -C cnn-super-resolution_amd`).

Device memory is passed as integer addresses, so torch tensors work
(`tensor.data_ptr()`), as do buffers from `malloc()` below.  torch is imported
first when available so that this library and torch share one HIP runtime.
"""
import ctypes
import os

try:  # share torch's HIP runtime (same SONAME) when torch is present
    import torch  # noqa: F401
except Exception:  # pragma: no cover - CLI-only environments
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LIB_PATH = os.environ.get("SRCNN_HIP_LIB", os.path.join(PKG, "lib", "libsrcnn_hip.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError("libsrcnn_hip.so not built at %s (run `make -C %s`)" % (LIB_PATH, PKG))

_lib = ctypes.CDLL(LIB_PATH)

_P = ctypes.c_void_p
_U = ctypes.c_uint32
_I = ctypes.c_int
_F = ctypes.c_float
_S = ctypes.c_size_t


class Net(ctypes.Structure):
    """srcnn_net: Config n1, n2, f1, f2, f3 (reference src/Config.hpp:27-28)."""
    _fields_ = [("n1", _U), ("n2", _U), ("f1", _U), ("f2", _U), ("f3", _U)]

    def __repr__(self):
        return "Net(n1=%d, n2=%d, f1=%d, f2=%d, f3=%d)" % (self.n1, self.n2, self.f1, self.f2, self.f3)


_NP = ctypes.POINTER(Net)


class YuvFrame(ctypes.Structure):
    """srcnn_yuv_frame: the device addresses of a frame's y, u and v planes and
    the pitches in bytes of y and of u / v."""
    _fields_ = [("y", _P), ("u", _P), ("v", _P), ("pitch_y", _U), ("pitch_c", _U)]


_FP = ctypes.POINTER(YuvFrame)


class YuvFormat(ctypes.Structure):
    """srcnn_yuv_format: bits per sample (8..16), msb (1: the value sits in the
    high bits of its 16-bit word, P010 style), layout (YUV_PLANAR or
    YUV_SEMIPLANAR), the chroma subsampling cx x cy and the range."""
    _fields_ = [("bits", _U), ("msb", _U), ("layout", _U), ("cx", _U), ("cy", _U), ("range", ctypes.c_int32)]

    def __repr__(self):
        return "YuvFormat(bits=%d, msb=%d, layout=%d, cx=%d, cy=%d, range=%d)" % (
            self.bits, self.msb, self.layout, self.cx, self.cy, self.range)


_MP = ctypes.POINTER(YuvFormat)

# name -> (restype, argtypes); int restype = status code checked by _call
SIGNATURES = {
    "srcnn_abi_version": (_I, []),
    "srcnn_last_error": (ctypes.c_char_p, []),
    "srcnn_device_count": (_I, [ctypes.POINTER(_I)]),
    "srcnn_set_device": (_I, [_I]),
    "srcnn_device_name": (_I, [ctypes.c_char_p, _S]),
    "srcnn_malloc": (_I, [ctypes.POINTER(_P), _S]),
    "srcnn_free": (_I, [_P]),
    "srcnn_host_alloc": (_I, [ctypes.POINTER(_P), _S]),
    "srcnn_host_free": (_I, [_P]),
    "srcnn_memcpy_h2d": (_I, [_P, _P, _S, _P]),
    "srcnn_memcpy_d2h": (_I, [_P, _P, _S, _P]),
    "srcnn_memcpy_d2d": (_I, [_P, _P, _S, _P]),
    "srcnn_fill_f32": (_I, [_P, _F, _S, _P]),
    "srcnn_stream_create": (_I, [ctypes.POINTER(_P)]),
    "srcnn_stream_destroy": (_I, [_P]),
    "srcnn_stream_sync": (_I, [_P]),
    "srcnn_device_sync": (_I, []),
    "srcnn_event_create": (_I, [ctypes.POINTER(_P)]),
    "srcnn_event_destroy": (_I, [_P]),
    "srcnn_event_record": (_I, [_P, _P]),
    "srcnn_event_sync": (_I, [_P]),
    "srcnn_event_elapsed_ms": (_I, [_P, _P, ctypes.POINTER(_F)]),
    "srcnn_graph_begin": (_I, [_P]),
    "srcnn_graph_end": (_I, [_P, ctypes.POINTER(_P)]),
    "srcnn_graph_launch": (_I, [_P, _P]),
    "srcnn_graph_destroy": (_I, [_P]),
    "srcnn_conv_fwd": (_I, [_P, _P, _P, _P, _U, _U, _U, _U, _U, _I, _U, _P]),
    "srcnn_last_delta": (_I, [_P, _P, _P, _U, _U, _U, _U, _U, _P]),
    "srcnn_conv_delta": (_I, [_P, _P, _P, _P, _U, _U, _U, _U, _U, _U, _P]),
    "srcnn_conv_grad_workspace_bytes": (_S, [_U, _U, _U, _U, _U, _U]),
    "srcnn_conv_grad_acc": (_I, [_P, _P, _P, _P, _U, _U, _U, _U, _U, _U, _P, _S, _P]),
    "srcnn_sgd_update": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _U, _U, _U, _P]),
    "srcnn_reduce_workspace_bytes": (_S, [_S]),
    "srcnn_sq_err": (_I, [_P, _P, _P, _U, _U, _U, _U, _U, _P, _S, _P]),
    "srcnn_sum": (_I, [_P, _S, _I, _P, _P, _S, _P]),
    "srcnn_sub_scalar": (_I, [_P, _F, _S, _P]),
    "srcnn_sub_mean": (_I, [_P, _S, _P, _P, _S, _P]),
    "srcnn_extract_luma": (_I, [_P, _P, _U, _U, _I, _P]),
    "srcnn_swap_luma": (_I, [_P, _P, _P, _U, _U, _U, _U, _P]),
    "srcnn_upscale_luma": (_I, [_P, _P, _U, _U, _U, _U, _P]),
    "srcnn_upscale_compose": (_I, [_P, _P, _P, _U, _U, _U, _P]),
    "srcnn_yuv_upscale_luma": (_I, [_P, _U, _P, _U, _U, _U, _U, _I, _P]),
    "srcnn_upscale_planes_u8": (_I, [_P, _P, _U, _U, _U, _P, _P, _U, _U, _U, _U, _P]),
    "srcnn_yuv_compose_luma": (_I, [_P, _P, _U, _U, _U, _I, _P]),
    "srcnn_yuv_upscale_luma16": (_I, [_P, _U, _P, _U, _U, _U, _U, _U, _U, _I, _P]),
    "srcnn_yuv_compose_luma16": (_I, [_P, _P, _U, _U, _U, _U, _U, _I, _P]),
    "srcnn_upscale_planes": (_I, [_P, _P, _U, _U, _U, _P, _P, _U, _U, _U, _U, _U, _U, _U, _P]),
    "srcnn_resize_luma": (_I, [_P, _P, _U, _U, _U, _U, _U, _P]),
    "srcnn_resize_compose": (_I, [_P, _P, _P, _U, _U, _U, _U, _P]),
    "srcnn_yuv_resize_luma": (_I, [_P, _U, _P, _U, _U, _U, _U, _U, _U, _U, _I, _P]),
    "srcnn_resize_planes": (_I, [_P, _P, _U, _U, _U, _P, _P, _U, _U, _U, _U, _U, _U, _U, _U, _U, _U, _P]),
    "srcnn_downscale_rgba": (_I, [_P, _P, _U, _U, _U, _P]),
    "srcnn_gather_tiles": (_I, [_P, _U, _U, _U, _U, _U, _U, _U, _U, _U, _I, _P, _P, _P]),
    "srcnn_gather_batch": (_I, [_P, _U, _P, _U, _U, _U, _P, _P, _P, _P]),
    "srcnn_make_pairs_count": (_S, [_U, _U, _U, _U, _U, ctypes.POINTER(_U), ctypes.POINTER(_U)]),
    "srcnn_make_pairs_workspace_bytes": (_S, [_U, _U, _U]),
    "srcnn_make_pairs": (_I, [_P, _U, _U, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_quality_workspace_bytes": (_S, [_U, _U, _U]),
    "srcnn_quality": (_I, [_P, _I, _U, _P, _I, _U, _U, _U, _U, _P, _P, _S, _P]),
    "srcnn_quality_frame_workspace_bytes": (_S, [_U, _U, _U, _U, _U]),
    "srcnn_quality_frame": (_I, [_MP, _FP, _MP, _FP, _U, _U, _U, _P, _P, _S, _P]),
    "srcnn_downscale_planes": (_I, [_P, _P, _U, _U, _U, _P, _P, _U, _U, _U, _U, _U, _U, _U, _P]),
    "srcnn_downscale_frame": (_I, [_MP, _FP, _FP, _U, _U, _U, _P]),
    "srcnn_make_pairs_frame_workspace_bytes": (_S, [_MP, _U, _U, _U]),
    "srcnn_make_pairs_frame": (_I, [_MP, _FP, _U, _U, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_evaluate_frame_workspace_bytes": (_S, [_NP, _MP, _U, _U, _U]),
    "srcnn_evaluate_frame": (_I, [_NP, _MP, _FP, _U, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_upscale_workspace_bytes": (_S, [_NP, _U, _U, _U]),
    "srcnn_upscale": (_I, [_NP, _P, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_upscale_yuv_workspace_bytes": (_S, [_NP, _U, _U, _U]),
    "srcnn_upscale_yuv": (_I, [_NP, _FP, _FP, _U, _U, _U, _U, _U, _I, _P, _P, _S, _P]),
    "srcnn_upscale_frame": (_I, [_NP, _MP, _FP, _FP, _U, _U, _U, _P, _P, _S, _P]),
    "srcnn_upscale_to_workspace_bytes": (_S, [_NP, _U, _U, _U, _U]),
    "srcnn_upscale_to": (_I, [_NP, _P, _U, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_upscale_frame_to_workspace_bytes": (_S, [_NP, _U, _U, _U, _U]),
    "srcnn_upscale_frame_to": (_I, [_NP, _MP, _FP, _FP, _U, _U, _U, _U, _P, _P, _S, _P]),
    "srcnn_evaluate_workspace_bytes": (_S, [_NP, _U, _U, _U]),
    "srcnn_evaluate": (_I, [_NP, _P, _U, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_net_offsets": (_I, [_NP, ctypes.POINTER(_S)]),
    "srcnn_net_param_count": (_S, [_NP]),
    "srcnn_train_workspace_bytes": (_S, [_NP, _U, _U, _U]),
    "srcnn_train_fwd_bwd": (_I, [_NP, _P, _P, _U, _U, _U, _P, _P, _P, _P, _S, _P]),
    "srcnn_update_all": (_I, [_NP, _P, _P, _P, _F, _F, ctypes.POINTER(_F), _U, _P]),
    "srcnn_train_step": (_I, [_NP, _P, _P, _U, _U, _U, _P, _P, _P, _F, _F, ctypes.POINTER(_F), _U,
                              _P, _P, _S, _P]),
    "srcnn_train_fwd_bwd_lazy": (_I, [_NP, _P, _P, _U, _U, _U, _P, _P, _P, _P, _P, _F, _F,
                                      ctypes.POINTER(_F), _U, _P, _P, _S, _P]),
    "srcnn_train_activations":(_I, [_NP, _U, _U, _U, _P, _S, _P, _P, _P, _P]),
    "srcnn_preload": (_I, [_NP]),
    "srcnn_forward_workspace_bytes": (_S, [_NP, _U, _U, _U]),
    "srcnn_forward": (_I, [_NP, _P, _U, _U, _U, _P, _P, _P, _S, _P]),
    "srcnn_profile_enable": (_I, [_I]),
    "srcnn_profile_reset": (_I, []),
    "srcnn_profile_count": (_I, [ctypes.POINTER(_I)]),
    "srcnn_profile_get": (_I, [_I, ctypes.c_char_p, _S, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.POINTER(ctypes.c_double)]),
    "srcnn_profile_print": (_I, []),
    "srcnn_profile_clock": (_I, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]),
    "srcnn_set_path": (_I, [_I]),
    "srcnn_set_arith": (_I, [_I]),
    "srcnn_get_arith": (_I, []),
    "srcnn_get_path": (_I, []),
    "srcnn_last_path": (ctypes.c_char_p, []),
    "srcnn_last_kernels": (ctypes.c_char_p, []),
    "srcnn_comm_id": (_I, [ctypes.c_char_p]),
    "srcnn_comm_init_rank": (_I, [ctypes.POINTER(_P), _I, ctypes.c_char_p, _I]),
    "srcnn_comm_init_all": (_I, [ctypes.POINTER(_P), _I, ctypes.POINTER(_I)]),
    "srcnn_comm_destroy": (_I, [_P]),
    "srcnn_comm_rank": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "srcnn_comm_group_start": (_I, []),
    "srcnn_comm_group_end": (_I, []),
    "srcnn_allreduce_grads": (_I, [_P, _P, _S, _P]),
    "srcnn_comm_version": (_I, [ctypes.POINTER(_I), ctypes.c_char_p, _S]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(_lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


class SrcnnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("srcnn error %d: %s" % (code, msg))
        self.code = code


OK, ERR_INVALID, ERR_HIP, ERR_WORKSPACE, ERR_ALLOC, ERR_COMM = 0, -1, -2, -3, -4, -5
COMM_ID_BYTES = 128
# pixel formats of srcnn_quality (SRCNN_PIX_*)
PIX_LUMA_F32, PIX_RGB8, PIX_RGBA8 = 1, 3, 4
# range of a Y'CbCr frame's luma (SRCNN_YUV_*)
YUV_LIMITED, YUV_FULL = 0, 1
# chroma layout of a frame (SRCNN_YUV_*): two planes, or one plane of (U, V) pairs
YUV_PLANAR, YUV_SEMIPLANAR = 0, 1


def _call(name, *args):
    rc = getattr(_lib, name)(*args)
    if rc != 0:
        raise SrcnnError(rc, _lib.srcnn_last_error().decode())
    return rc


def lib():
    return _lib


def last_error():
    return _lib.srcnn_last_error().decode()


def abi_version():
    return _lib.srcnn_abi_version()


def exported_symbols():
    return list(SIGNATURES)


def ptr(t):
    """Device address of a torch tensor / int / None."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def cur_stream():
    """hipStream_t of torch's current stream (0 = default)."""
    if torch is None:
        return None
    return torch.cuda.current_stream().cuda_stream


# ---- runtime ----
def device_count():
    c = _I()
    _call("srcnn_device_count", ctypes.byref(c))
    return c.value


def set_device(d):
    _call("srcnn_set_device", d)


def device_name():
    buf = ctypes.create_string_buffer(256)
    _call("srcnn_device_name", buf, 256)
    return buf.value.decode()


def malloc(nbytes):
    p = _P()
    _call("srcnn_malloc", ctypes.byref(p), nbytes)
    return p.value or 0


def free(p):
    _call("srcnn_free", p)


def stream_create():
    s = _P()
    _call("srcnn_stream_create", ctypes.byref(s))
    return s.value


def stream_sync(s=None):
    _call("srcnn_stream_sync", s)


def event_create():
    e = _P()
    _call("srcnn_event_create", ctypes.byref(e))
    return e.value


def event_record(e, s=None):
    _call("srcnn_event_record", e, s)


def event_sync(e):
    _call("srcnn_event_sync", e)


def event_elapsed_ms(a, b):
    ms = _F()
    _call("srcnn_event_elapsed_ms", a, b, ctypes.byref(ms))
    return ms.value


def event_destroy(e):
    _call("srcnn_event_destroy", e)


def host_alloc(nbytes):
    """Address of nbytes of page-locked host memory (srcnn_host_alloc)."""
    p = _P()
    _call("srcnn_host_alloc", ctypes.byref(p), nbytes)
    return p.value or 0


def host_free(p):
    _call("srcnn_host_free", p)


def memcpy_h2d(dst, src_addr, nbytes, s=None):
    _call("srcnn_memcpy_h2d", dst, src_addr, nbytes, s)


def memcpy_d2h(dst_addr, src, nbytes, s=None):
    _call("srcnn_memcpy_d2h", dst_addr, src, nbytes, s)


def fill_f32(dst, value, count, s=None):
    _call("srcnn_fill_f32", ptr(dst), value, count, s)


# ---- operators (argument order = include/srcnn.h) ----
def conv_fwd(inp, out, W, B, in_w, in_h, n_prev, n_cur, f, relu, batch, s=None):
    _call("srcnn_conv_fwd", ptr(inp), ptr(out), ptr(W), ptr(B), in_w, in_h, n_prev, n_cur, f,
          int(relu), batch, s)


def last_delta(gt, y, d, gt_w, gt_h, out_w, out_h, batch, s=None):
    _call("srcnn_last_delta", ptr(gt), ptr(y), ptr(d), gt_w, gt_h, out_w, out_h, batch, s)


def conv_delta(d_next, y_curr, d_curr, W_next, f_next, n_curr, n_next, curr_w, curr_h, batch, s=None):
    _call("srcnn_conv_delta", ptr(d_next), ptr(y_curr), ptr(d_curr), ptr(W_next), f_next, n_curr,
          n_next, curr_w, curr_h, batch, s)


def conv_grad_workspace_bytes(n_prev, n_cur, f, out_w, out_h, batch):
    return _lib.srcnn_conv_grad_workspace_bytes(n_prev, n_cur, f, out_w, out_h, batch)


def conv_grad_acc(inp, delta, gW, gB, n_prev, n_cur, f, out_w, out_h, batch, ws, ws_bytes, s=None):
    _call("srcnn_conv_grad_acc", ptr(inp), ptr(delta), ptr(gW), ptr(gB), n_prev, n_cur, f, out_w,
          out_h, batch, ptr(ws), ws_bytes, s)


def sgd_update(W, B, gW, gB, dW, dB, momentum, wd, lr, batch, nW, nB, s=None):
    _call("srcnn_sgd_update", ptr(W), ptr(B), ptr(gW), ptr(gB), ptr(dW), ptr(dB), momentum, wd, lr,
          batch, nW, nB, s)


def reduce_workspace_bytes(n):
    return _lib.srcnn_reduce_workspace_bytes(n)


def sq_err(gt, y, result, gt_w, gt_h, out_w, out_h, batch, ws, ws_bytes, s=None):
    _call("srcnn_sq_err", ptr(gt), ptr(y), ptr(result), gt_w, gt_h, out_w, out_h, batch, ptr(ws),
          ws_bytes, s)


def buf_sum(data, n, squared, result, ws, ws_bytes, s=None):
    _call("srcnn_sum", ptr(data), n, int(squared), ptr(result), ptr(ws), ws_bytes, s)


def sub_scalar(data, value, n, s=None):
    _call("srcnn_sub_scalar", ptr(data), value, n, s)


def sub_mean(data, n, mean, ws, ws_bytes, s=None):
    _call("srcnn_sub_mean", ptr(data), n, ptr(mean), ptr(ws), ws_bytes, s)


def extract_luma(rgba, luma, w, h, normalize, s=None):
    _call("srcnn_extract_luma", ptr(rgba), ptr(luma), w, h, int(normalize), s)


def swap_luma(rgba, new_luma, rgb, w, h, luma_w, luma_h, s=None):
    _call("srcnn_swap_luma", ptr(rgba), ptr(new_luma), ptr(rgb), w, h, luma_w, luma_h, s)


def upscale_luma(rgba, luma_padded, w, h, scale, pad, s=None):
    """rgba [h][w][4] u8 -> bicubic x scale luma, edge-replicated into the
    padded plane [(scale*h+pad)][(scale*w+pad)] f32 (srcnn_upscale_luma)."""
    _call("srcnn_upscale_luma", ptr(rgba), ptr(luma_padded), w, h, scale, pad, s)


def upscale_compose(rgba, new_luma, rgb, w, h, scale, s=None):
    """bicubic x scale of the source's r, g, b + new_luma [scale*h][scale*w]
    -> rgb [scale*h][scale*w][3] u8 (srcnn_upscale_compose)."""
    _call("srcnn_upscale_compose", ptr(rgba), ptr(new_luma), ptr(rgb), w, h, scale, s)


def yuv_upscale_luma(y, pitch_y, luma_padded, w, h, scale, pad, yuv_range, s=None):
    """Y [h][w] u8 (rows pitch_y bytes apart) -> the bicubic x scale of its
    luma (YUV_FULL: Y/255, YUV_LIMITED: (Y-16)/219), edge-replicated into the
    padded plane [(scale*h+pad)][(scale*w+pad)] f32 (srcnn_yuv_upscale_luma)."""
    _call("srcnn_yuv_upscale_luma", ptr(y), pitch_y, ptr(luma_padded), w, h, scale, pad, yuv_range, s)


def upscale_planes_u8(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, scale, s=None):
    """Two u8 planes [ph][pw] -> the top-left ow x oh of the bicubic x scale of
    each, rounded to nearest and clamped, into two u8 planes
    (srcnn_upscale_planes_u8)."""
    _call("srcnn_upscale_planes_u8", ptr(src0), ptr(src1), src_pitch, pw, ph, ptr(dst0), ptr(dst1),
          dst_pitch, ow, oh, scale, s)


def yuv_compose_luma(luma, y, pitch_y, W, H, yuv_range, s=None):
    """luma [H][W] f32 -> Y [H][W] u8, rows pitch_y bytes apart
    (srcnn_yuv_compose_luma)."""
    _call("srcnn_yuv_compose_luma", ptr(luma), ptr(y), pitch_y, W, H, yuv_range, s)


def yuv_upscale_luma16(y, pitch_y, luma_padded, w, h, scale, pad, bits, msb, yuv_range, s=None):
    """yuv_upscale_luma for samples of `bits` (8..16) bits: one byte at 8 bits,
    else a 16-bit word with the value in its low (msb 0) or high (msb 1) bits;
    pitch_y in bytes (srcnn_yuv_upscale_luma16)."""
    _call("srcnn_yuv_upscale_luma16", ptr(y), pitch_y, ptr(luma_padded), w, h, scale, pad, bits, msb, yuv_range, s)


def yuv_compose_luma16(luma, y, pitch_y, W, H, bits, msb, yuv_range, s=None):
    """luma [H][W] f32 -> Y [H][W] samples of `bits` bits, rows pitch_y bytes
    apart (srcnn_yuv_compose_luma16)."""
    _call("srcnn_yuv_compose_luma16", ptr(luma), ptr(y), pitch_y, W, H, bits, msb, yuv_range, s)


def upscale_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, scale, bits, msb, layout, s=None):
    """A frame's chroma [ph][pw] -> the top-left ow x oh of its bicubic x scale,
    rounded and clamped to `bits` bits: YUV_PLANAR: two planes in, two out;
    YUV_SEMIPLANAR: src0 / dst0 hold (U, V) pairs, src1 and dst1 are None;
    pitches in bytes (srcnn_upscale_planes)."""
    _call("srcnn_upscale_planes", ptr(src0), ptr(src1), src_pitch, pw, ph, ptr(dst0), ptr(dst1), dst_pitch, ow, oh,
          scale, bits, msb, layout, s)


def resize_luma(rgba, luma_padded, w, h, W, H, pad, s=None):
    """upscale_luma to any output size W x H, w <= W <= 4w and h <= H <= 4h:
    the padded plane [(H+pad)][(W+pad)] f32 (srcnn_resize_luma)."""
    _call("srcnn_resize_luma", ptr(rgba), ptr(luma_padded), w, h, W, H, pad, s)


def resize_compose(rgba, new_luma, rgb, w, h, W, H, s=None):
    """upscale_compose to any output size: rgba [h][w][4] u8 + new_luma [H][W]
    f32 -> rgb [H][W][3] u8 (srcnn_resize_compose)."""
    _call("srcnn_resize_compose", ptr(rgba), ptr(new_luma), ptr(rgb), w, h, W, H, s)


def yuv_resize_luma(y, pitch_y, luma_padded, w, h, W, H, pad, bits, msb, yuv_range, s=None):
    """yuv_upscale_luma16 to any output size: Y [h][w] of `bits` bits ->
    the padded plane [(H+pad)][(W+pad)] f32 (srcnn_yuv_resize_luma)."""
    _call("srcnn_yuv_resize_luma", ptr(y), pitch_y, ptr(luma_padded), w, h, W, H, pad, bits, msb, yuv_range, s)


def resize_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, rx_num, rx_den, ry_num, ry_den,
                  bits, msb, layout, s=None):
    """upscale_planes at the explicit ratios rx_num / rx_den and ry_num / ry_den
    (the source step per output sample; a frame's chroma takes the luma's w / W
    and h / H): [ph][pw] -> [oh][ow], ow <= ceil(pw * rx_den / rx_num), rows
    likewise (srcnn_resize_planes)."""
    _call("srcnn_resize_planes", ptr(src0), ptr(src1), src_pitch, pw, ph, ptr(dst0), ptr(dst1), dst_pitch, ow, oh,
          rx_num, rx_den, ry_num, ry_den, bits, msb, layout, s)


def downscale_rgba(rgba, small, W, H, scale, s=None):
    """rgba [H][W][4] u8 -> antialiased bicubic / scale, small
    [H//scale][W//scale][4] u8, alpha 255 (srcnn_downscale_rgba)."""
    _call("srcnn_downscale_rgba", ptr(rgba), ptr(small), W, H, scale, s)


def gather_tiles(plane, pw, ph, x0, y0, stride, nx, ny, tw, th, sub_mean, tiles, means=None, s=None):
    """plane [ph][pw] f32 -> tiles [nx*ny][th][tw], tile iy*nx + ix from
    (x0 + ix*stride, y0 + iy*stride); with sub_mean each minus its own mean,
    which means [nx*ny] (may be None) then receives (srcnn_gather_tiles)."""
    _call("srcnn_gather_tiles", ptr(plane), pw, ph, x0, y0, stride, nx, ny, tw, th, int(sub_mean),
          ptr(tiles), ptr(means), s)


def pack_plane_table(pairs):
    """[(x, t, x_pitch, t_pitch, w, h), ...] (x, t: tensors or device
    addresses) -> the srcnn_plane_pair table as a uint8 numpy array: 32 bytes
    per entry, little-endian {u64 x, u64 t, u32 x_pitch, t_pitch, w, h}.
    Upload it; the tensors must outlive its use."""
    import numpy as np
    table = np.zeros(len(pairs), dtype=np.dtype([("x", "<u8"), ("t", "<u8"), ("x_pitch", "<u4"),
                                                 ("t_pitch", "<u4"), ("w", "<u4"), ("h", "<u4")]))
    for i, (x, t, x_pitch, t_pitch, w, h) in enumerate(pairs):
        table[i] = (ptr(x), ptr(t), x_pitch, t_pitch, w, h)
    return table.view(np.uint8).reshape(-1)


def pack_tile_refs(refs):
    """[n][4] integers {plane, x, y, op} -> the srcnn_tile_ref records as a
    uint8 numpy array: 16 bytes each, four little-endian u32."""
    import numpy as np
    a = np.asarray(refs)
    if a.size == 0:
        return np.zeros(0, np.uint8)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("pack_tile_refs: expected an array [n][4], got shape %s" % (a.shape,))
    if (a < 0).any() or (a > 0xffffffff).any():
        raise ValueError("pack_tile_refs: a field does not fit 32 unsigned bits")
    return np.ascontiguousarray(a.astype("<u4")).view(np.uint8).reshape(-1)


def gather_batch(planes, n_planes, refs, n, tw, th, X, T, means=None, s=None):
    """planes (device srcnn_plane_pair table, pack_plane_table) and refs
    (device srcnn_tile_ref records, pack_tile_refs) -> X, T [n][th][tw] f32:
    record i's footprint through its orientation, X minus the footprint's
    mean, which means [n] (may be None) receives; an invalid record gives NaN
    tiles (srcnn_gather_batch)."""
    _call("srcnn_gather_batch", ptr(planes), n_planes, ptr(refs), n, tw, th, ptr(X), ptr(T), ptr(means), s)


def make_pairs_count(W, H, scale, tile, stride):
    """(count, nx, ny) of the tile grid srcnn_make_pairs cuts; count 0 if the
    image is too small or an argument is invalid."""
    nx, ny = _U(), _U()
    n = _lib.srcnn_make_pairs_count(W, H, scale, tile, stride, ctypes.byref(nx), ctypes.byref(ny))
    return n, nx.value, ny.value


def make_pairs_workspace_bytes(W, H, scale):
    return _lib.srcnn_make_pairs_workspace_bytes(W, H, scale)


def make_pairs(rgba, W, H, scale, tile, stride, X, T, ws, ws_bytes, s=None):
    """Full-size rgba [H][W][4] u8 -> X, T [count][tile][tile] f32
    (srcnn_make_pairs): downscale_rgba, upscale_luma (pad 0), extract_luma,
    gather_tiles with the mean (X) and without (T)."""
    _call("srcnn_make_pairs", ptr(rgba), W, H, scale, tile, stride, ptr(X), ptr(T), ptr(ws),
          ws_bytes, s)


def quality_workspace_bytes(W, H, shave=0):
    return _lib.srcnn_quality_workspace_bytes(W, H, shave)


def quality(a, fmt_a, pitch_a, b, fmt_b, pitch_b, W, H, shave, result, ws, ws_bytes, s=None):
    """{mse, psnr, ssim} (3 doubles, device) of the luma of two W x H images,
    each PIX_RGB8 / PIX_RGBA8 / PIX_LUMA_F32 with its own pitch in pixels,
    `shave` pixels dropped per side (srcnn_quality)."""
    _call("srcnn_quality", ptr(a), fmt_a, pitch_a, ptr(b), fmt_b, pitch_b, W, H, shave, ptr(result),
          ptr(ws), ws_bytes, s)


# ---- network level ----
def net_offsets(net):
    arr = (_S * 6)()
    _call("srcnn_net_offsets", ctypes.byref(net), arr)
    return list(arr)


def net_param_count(net):
    return _lib.srcnn_net_param_count(ctypes.byref(net))


def train_workspace_bytes(net, w, h, batch):
    return _lib.srcnn_train_workspace_bytes(ctypes.byref(net), w, h, batch)


def train_fwd_bwd(net, X, T, w, h, batch, params, grads, sq_err_dev, ws, ws_bytes, s=None):
    _call("srcnn_train_fwd_bwd", ctypes.byref(net), ptr(X), ptr(T), w, h, batch, ptr(params),
          ptr(grads), ptr(sq_err_dev), ptr(ws), ws_bytes, s)


def update_all(net, params, grads, mom, momentum, wd, lr, batch, s=None):
    lr_arr = (_F * 3)(*lr)
    _call("srcnn_update_all", ctypes.byref(net), ptr(params), ptr(grads), ptr(mom), momentum, wd,
          lr_arr, batch, s)


def train_step(net, X, T, w, h, batch, params, grads, mom, momentum, wd, lr, update_batch,
               sq_err_dev, ws, ws_bytes, s=None):
    """srcnn_train_step: train_fwd_bwd + update_all on one device (the update
    fused into the gradient reduction on the fused path)."""
    lr_arr = (_F * 3)(*lr)
    _call("srcnn_train_step", ctypes.byref(net), ptr(X), ptr(T), w, h, batch, ptr(params),
          ptr(grads), ptr(mom), momentum, wd, lr_arr, update_batch, ptr(sq_err_dev), ptr(ws),
          ws_bytes, s)


def train_fwd_bwd_lazy(net, X, T, w, h, batch, params_in, params_out, mom_in, mom_out, grads,
                       momentum, wd, lr, update_batch, sq_err_dev, ws, ws_bytes, s=None):
    """srcnn_train_fwd_bwd_lazy: the pending update of `grads` (update_batch
    > 0) out of place into params_out / mom_out, then this step's gradients
    over the batch on the updated parameters, written to `grads`."""
    lr_arr = (_F * 3)(*lr)
    _call("srcnn_train_fwd_bwd_lazy", ctypes.byref(net), ptr(X), ptr(T), w, h, batch, ptr(params_in),
          ptr(params_out), ptr(mom_in), ptr(mom_out), ptr(grads), momentum, wd, lr_arr, update_batch,
          ptr(sq_err_dev), ptr(ws), ws_bytes, s)


class Graph:
    """A replayable HIP graph of the library calls `fn()` enqueues on `stream`
    (srcnn_graph_begin / _end); `launch()` replays it on the same stream."""

    def __init__(self, fn, stream):
        if not stream:
            raise ValueError("graph capture needs a created stream (not the NULL stream)")
        self.stream = stream
        self.handle = _P()
        _call("srcnn_graph_begin", stream)
        try:
            fn()
        finally:
            _call("srcnn_graph_end", stream, ctypes.byref(self.handle))

    def launch(self):
        _call("srcnn_graph_launch", self.handle, self.stream)

    def close(self):
        if self.handle:
            _call("srcnn_graph_destroy", self.handle)
            self.handle = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_activations(net, w, h, batch, ws, ws_bytes, A1, A2, A3, s=None):
    """srcnn_train_activations: the last training call's activations of the
    three layers in `ws`, copied out in the reference HWC layout."""
    _call("srcnn_train_activations", ctypes.byref(net), w, h, batch, ptr(ws), ws_bytes, ptr(A1),
          ptr(A2), ptr(A3), s)


def forward_workspace_bytes(net, w, h, batch):
    return _lib.srcnn_forward_workspace_bytes(ctypes.byref(net), w, h, batch)


def forward(net, X, w, h, batch, params, out, ws, ws_bytes, s=None):
    _call("srcnn_forward", ctypes.byref(net), ptr(X), w, h, batch, ptr(params), ptr(out), ptr(ws),
          ws_bytes, s)


def upscale_workspace_bytes(net, w, h, scale):
    return _lib.srcnn_upscale_workspace_bytes(ctypes.byref(net), w, h, scale)


def upscale(net, rgba, w, h, scale, params, rgb, ws, ws_bytes, s=None):
    """Low-resolution rgba [h][w][4] u8 -> super-resolved rgb
    [scale*h][scale*w][3] u8 (srcnn_upscale): upscale_luma, sub_mean over the
    padded plane, forward, upscale_compose."""
    _call("srcnn_upscale", ctypes.byref(net), ptr(rgba), w, h, scale, ptr(params), ptr(rgb),
          ptr(ws), ws_bytes, s)


def upscale_yuv_workspace_bytes(net, w, h, scale):
    return _lib.srcnn_upscale_yuv_workspace_bytes(ctypes.byref(net), w, h, scale)


def yuv_frame(y, u, v, pitch_y, pitch_c):
    """A YuvFrame of three device planes (torch tensors or addresses)."""
    return YuvFrame(ptr(y), ptr(u), ptr(v), pitch_y, pitch_c)


def upscale_yuv(net, src, dst, w, h, cx, cy, scale, yuv_range, params, ws, ws_bytes, s=None):
    """One planar Y'CbCr frame (src, a YuvFrame: w x h luma, chroma subsampled
    by cx x cy) -> the frame scale times as large (dst) (srcnn_upscale_yuv):
    yuv_upscale_luma, sub_mean over the padded plane, forward,
    yuv_compose_luma, and upscale_planes_u8 for the chroma."""
    _call("srcnn_upscale_yuv", ctypes.byref(net), ctypes.byref(src), ctypes.byref(dst), w, h, cx, cy,
          scale, yuv_range, ptr(params), ptr(ws), ws_bytes, s)


def yuv_format(bits=8, msb=0, layout=YUV_PLANAR, cx=2, cy=2, yuv_range=YUV_LIMITED):
    """A YuvFormat; the defaults are 8-bit planar 4:2:0 at limited range."""
    return YuvFormat(bits, msb, layout, cx, cy, yuv_range)


def upscale_frame(net, fmt, src, dst, w, h, scale, params, ws, ws_bytes, s=None):
    """upscale_yuv for every YuvFormat: 8 to 16 bits per sample, planar or
    semi-planar (NV12, P010: the frames' u holds the (U, V) pairs, v is None);
    the workspace is upscale_yuv_workspace_bytes (srcnn_upscale_frame)."""
    _call("srcnn_upscale_frame", ctypes.byref(net), ctypes.byref(fmt) if fmt is not None else None,
          ctypes.byref(src), ctypes.byref(dst), w, h, scale, ptr(params), ptr(ws), ws_bytes, s)


def quality_frame_workspace_bytes(w, h, cx=2, cy=2, shave=0):
    return _lib.srcnn_quality_frame_workspace_bytes(w, h, cx, cy, shave)


def quality_frame(fmt_a, a, fmt_b, b, w, h, shave, result, ws, ws_bytes, s=None):
    """{mse_y, psnr_y, ssim_y, mse_u, psnr_u, mse_v, psnr_v, psnr_all} (8
    doubles, device) of two Y'CbCr frames of w x h luma samples, each a
    YuvFrame with its own YuvFormat (equal bits, cx, cy and range; msb, layout
    and pitches may differ), `shave` luma pixels dropped per side: PSNR of the
    integer code values per plane, SSIM on luma (srcnn_quality_frame)."""
    ref = lambda x: ctypes.byref(x) if x is not None else None
    _call("srcnn_quality_frame", ref(fmt_a), ref(a), ref(fmt_b), ref(b), w, h, shave, ptr(result), ptr(ws),
          ws_bytes, s)


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def downscale_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, scale, bits, msb, layout, s=None):
    """A frame's planes [ph][pw] of `bits`-bit samples -> the antialiased
    bicubic / scale of the code values, [oh][ow] with ow <= ceil(pw / scale),
    oh likewise, rounded to nearest even and clamped.  YUV_PLANAR: one plane
    (src1 and dst1 None) or two; YUV_SEMIPLANAR: src0 / dst0 hold (U, V)
    pairs; pitches in bytes (srcnn_downscale_planes)."""
    _call("srcnn_downscale_planes", ptr(src0), ptr(src1), src_pitch, pw, ph, ptr(dst0), ptr(dst1), dst_pitch, ow,
          oh, scale, bits, msb, layout, s)


def downscale_frame(fmt, src, dst, W, H, scale, s=None):
    """One Y'CbCr frame of W x H luma samples (src, a YuvFrame) -> the frame
    W // scale x H // scale in the same YuvFormat (dst): downscale_planes of
    the luma, then of the chroma (srcnn_downscale_frame)."""
    _call("srcnn_downscale_frame", _ref(fmt), _ref(src), _ref(dst), W, H, scale, s)


def make_pairs_frame_workspace_bytes(fmt, W, H, scale):
    return _lib.srcnn_make_pairs_frame_workspace_bytes(_ref(fmt), W, H, scale)


def make_pairs_frame(fmt, frame, W, H, scale, tile, stride, X, T, ws, ws_bytes, s=None):
    """The luma of a Y'CbCr frame -> X, T [count][tile][tile] f32
    (srcnn_make_pairs_frame): downscale_planes of Y, yuv_upscale_luma16 of the
    small plane (pad 0) and of Y itself at scale 1, gather_tiles with the mean
    (X) and without (T).  Only frame.y is read."""
    _call("srcnn_make_pairs_frame", _ref(fmt), _ref(frame), W, H, scale, tile, stride, ptr(X), ptr(T), ptr(ws),
          ws_bytes, s)


def evaluate_frame_workspace_bytes(net, fmt, W, H, scale):
    return _lib.srcnn_evaluate_frame_workspace_bytes(_ref(net), _ref(fmt), W, H, scale)


def evaluate_frame(net, fmt, truth, W, H, scale, shave, params, result, ws, ws_bytes, s=None):
    """Full-size truth frame -> result (16 doubles, device): quality_frame's
    eight values of the net's x scale result, then of plain bicubic's
    (srcnn_evaluate_frame): downscale_frame, upscale_frame, quality_frame,
    yuv_upscale_luma16 (pad 0), yuv_compose_luma16, quality_frame."""
    _call("srcnn_evaluate_frame", _ref(net), _ref(fmt), _ref(truth), W, H, scale, shave, ptr(params), ptr(result),
          ptr(ws), ws_bytes, s)


def upscale_to_workspace_bytes(net, w, h, W, H):
    return _lib.srcnn_upscale_to_workspace_bytes(ctypes.byref(net), w, h, W, H)


def upscale_to(net, rgba, w, h, W, H, params, rgb, ws, ws_bytes, s=None):
    """upscale to any output size W x H within [1x, 4x] of w x h per axis
    (srcnn_upscale_to): resize_luma, sub_mean over the padded plane, forward,
    resize_compose."""
    _call("srcnn_upscale_to", ctypes.byref(net), ptr(rgba), w, h, W, H, ptr(params), ptr(rgb), ptr(ws), ws_bytes, s)


def upscale_frame_to_workspace_bytes(net, w, h, W, H):
    return _lib.srcnn_upscale_frame_to_workspace_bytes(ctypes.byref(net), w, h, W, H)


def upscale_frame_to(net, fmt, src, dst, w, h, W, H, params, ws, ws_bytes, s=None):
    """upscale_frame to any output size W x H within [1x, 4x] of w x h per axis
    (srcnn_upscale_frame_to): yuv_resize_luma, sub_mean, forward,
    yuv_compose_luma16, and resize_planes at the luma's ratios for the chroma."""
    _call("srcnn_upscale_frame_to", ctypes.byref(net), ctypes.byref(fmt) if fmt is not None else None,
          ctypes.byref(src), ctypes.byref(dst), w, h, W, H, ptr(params), ptr(ws), ws_bytes, s)


def evaluate_workspace_bytes(net, W, H, scale):
    return _lib.srcnn_evaluate_workspace_bytes(ctypes.byref(net), W, H, scale)


def evaluate(net, rgba, W, H, scale, shave, params, result, ws, ws_bytes, s=None):
    """Full-size ground truth rgba [H][W][4] u8 -> result (6 doubles, device):
    {mse, psnr, ssim} of the net's x scale result, then of plain bicubic's
    (srcnn_evaluate): downscale_rgba, upscale, quality, upscale_luma (pad 0),
    upscale_compose, quality."""
    _call("srcnn_evaluate", ctypes.byref(net), ptr(rgba), W, H, scale, shave, ptr(params),
          ptr(result), ptr(ws), ws_bytes, s)


def set_path(p):
    _call("srcnn_set_path", p)


def set_arith(a):
    """0: split-bf16 matrix-core products (default), 1: fp32 MFMA only."""
    _call("srcnn_set_arith", a)


def get_arith():
    return _lib.srcnn_get_arith()


def get_path():
    return _lib.srcnn_get_path()


def preload(net):
    """Resolve the net's gfx950 kernels on the current device (srcnn_preload):
    the runtime's lazy kernel setup happens here, not in the first step."""
    _call("srcnn_preload", ctypes.byref(net))


def last_kernels():
    """Kernel variants of this thread's most recent training call, as a list
    (srcnn_last_kernels), e.g. ["l12_fwd", "l3r_delta", "d1c_grad12", ...]."""
    v = _lib.srcnn_last_kernels().decode()
    return v.split(",") if v else []


def last_path():
    """Kernel family of this thread's most recent conv / network call:
    "fused", "wide", "fast", "generic" or "" (srcnn_last_path)."""
    return _lib.srcnn_last_path().decode()


# ---- multi-GPU: RCCL gradient reduction (srcnn_comm_*, srcnn_allreduce_grads) ----
def comm_id():
    """128-byte RCCL unique id (ncclGetUniqueId), made on ONE rank."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _call("srcnn_comm_id", buf)
    return buf.raw


def comm_init_rank(nranks, uid, rank):
    """Communicator of `rank` on the current device (one process per GPU)."""
    if len(uid) != COMM_ID_BYTES:
        raise ValueError("comm id must be %d bytes" % COMM_ID_BYTES)
    c = _P()
    _call("srcnn_comm_init_rank", ctypes.byref(c), nranks, uid, rank)
    return c.value


def comm_init_all(devices):
    """One communicator per device of one process (ncclCommInitAll)."""
    n = len(devices)
    comms = (_P * n)()
    devs = (_I * n)(*devices)
    _call("srcnn_comm_init_all", comms, n, devs)
    return list(comms)


def comm_destroy(c):
    _call("srcnn_comm_destroy", c)


def comm_rank(c):
    r, n = _I(), _I()
    _call("srcnn_comm_rank", c, ctypes.byref(r), ctypes.byref(n))
    return r.value, n.value


def comm_version():
    """(RCCL version code, path of the librccl the library is bound to)."""
    v = _I()
    buf = ctypes.create_string_buffer(4096)
    _call("srcnn_comm_version", ctypes.byref(v), buf, len(buf))
    return v.value, buf.value.decode()


def allreduce_grads(c, buf, count, s=None):
    """In-place sum of `count` floats over all ranks, on stream `s`."""
    _call("srcnn_allreduce_grads", c, ptr(buf), count, s)


# ---- profiling (reference `profile` mode) ----
def profile_enable(on=True):
    _call("srcnn_profile_enable", int(bool(on)))


def profile_reset():
    _call("srcnn_profile_reset")


def profile_stats():
    """{kernel name: (launches, total_ms)}; waits for recorded events."""
    n = _I()
    _call("srcnn_profile_count", ctypes.byref(n))
    out = {}
    buf = ctypes.create_string_buffer(256)
    for i in range(n.value):
        cnt, ms = ctypes.c_uint64(), ctypes.c_double()
        _call("srcnn_profile_get", i, buf, 256, ctypes.byref(cnt), ctypes.byref(ms))
        out[buf.value.decode()] = (cnt.value, ms.value)
    return out


def profile_clock(kernel):
    """Shader clock (GHz) held during the last launch of a fused kernel, or None."""
    ghz = ctypes.c_double()
    _call("srcnn_profile_clock", kernel.encode(), ctypes.byref(ghz))
    return ghz.value if ghz.value > 0 else None


def profile_print():
    _call("srcnn_profile_print")
