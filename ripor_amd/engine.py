"""Thin Python objects over the C ABI: device context, bound model weights, device trie, search.

torch is used only for device memory (tensors own the buffers whose ``data_ptr()`` crosses the
ABI) and for the current HIP stream handle. All compute happens in ``libripor_hip.so``.
"""
from __future__ import annotations

import ctypes as C
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import RiporHipError, check

_contexts: Dict[int, "Context"] = {}


def _stream_ptr(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Context:
    """One ``rpr_ctx`` per device (workspaces, KV cache and hipGraphs live in it)."""

    def __init__(self, device_index: int):
        if not torch.cuda.is_available():
            raise RiporHipError("no HIP device visible to torch: the search path has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device_index)
        h = C.c_void_p()
        check(self.lib.rpr_init(device_index, C.byref(h)), "rpr_init")
        self.handle = h

    @staticmethod
    def get(device=None) -> "Context":
        if device is None:
            idx = torch.cuda.current_device() if torch.cuda.is_available() else 0
        else:
            dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
            if dev.type != "cuda":
                raise RiporHipError(f"device {dev} is not a HIP device: the search path has no CPU fallback")
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if idx not in _contexts:
            _contexts[idx] = Context(idx)
        return _contexts[idx]

    def set_precision(self, name: str):
        """'f32' = exact fp32 MFMA; 'f16x2' = split-precision f16 MFMA (default)."""
        check(self.lib.rpr_set_precision(self.handle, {"f32": _lib.PREC_F32, "f16x2": _lib.PREC_F16X2, "bf16": _lib.PREC_BF16}[name]),
              "rpr_set_precision")

    def get_precision(self) -> str:
        return {_lib.PREC_F32: "f32", _lib.PREC_F16X2: "f16x2", _lib.PREC_BF16: "bf16"}[int(self.lib.rpr_get_precision(self.handle))]

    def has_bf16(self) -> bool:
        """The bf16 arithmetic of the training GEMMs (RPR_PREC_BF16) is compiled into this library."""
        return True

    def workspace_bytes(self) -> int:
        return int(self.lib.rpr_workspace_bytes(self.handle))

    def set_lane_split(self, min_rows: int):
        """Batches of at least ``min_rows`` decoder rows (queries x beams) run as two halves on two CU-masked streams
        (0 = never)."""
        check(self.lib.rpr_set_lane_split(self.handle, int(min_rows)), "rpr_set_lane_split")

    def lane_split(self) -> int:
        """The threshold in force; 0 when splitting is off or masked streams are unavailable."""
        return int(self.lib.rpr_lane_split(self.handle))

    def set_l0_table(self, mode: int):
        """The decoder's layer-0 Q/K/V table (``rpr_set_l0_table``): 0 = never, 1 = where the search would launch the
        projection on the 256 x 256 tile kernel (library default, same bits), 2 = always (tests)."""
        check(self.lib.rpr_set_l0_table(self.handle, int(mode)), "rpr_set_l0_table")

    def l0_table_bytes(self, model: "DeviceModel") -> int:
        """Size of the model's layer-0 Q/K/V table if the next search may read it, else 0."""
        return int(self.lib.rpr_l0_table_bytes(self.handle, model.handle))

    def set_gemm_mfma16(self, mode: int):
        """MFMA shape of the 256 x 256 split-precision GEMM (``rpr_set_gemm_mfma16``): 0 = 32x32x16 everywhere,
        1 = 16x16x32 in the tail passes of a search (library default; scores of forced sequences move in their last bits)."""
        check(self.lib.rpr_set_gemm_mfma16(self.handle, int(mode)), "rpr_set_gemm_mfma16")

    def gemm_mfma16(self) -> int:
        return int(self.lib.rpr_gemm_mfma16(self.handle))

    def set_tail_extras(self, mode: int):
        """Forced with extras (``rpr_set_tail_extras``): -1 = automatic (library default: more than 4096 decoder rows and
        fewer than 32 beams), 0 = off, n > 0 = always, with a budget of n extra sequences per query."""
        check(self.lib.rpr_set_tail_extras(self.handle, int(mode)), "rpr_set_tail_extras")

    def tail_extras(self) -> int:
        return int(self.lib.rpr_tail_extras(self.handle))

    def set_forced_tail(self, mode):
        """Forced-tail evaluation (``rpr_set_forced_tail``): queries whose beams can no longer be pruned leave the
        step-by-step loop at a fork and get their remaining positions scored in one teacher-forced pass.
        ``False``/0 = off, ``True``/1 = exact (library default), 2 = optimistic: no stage after the last fork; a query
        left unforced there raises ``STATUS_TAIL_LEFTOVER`` and the call must be repeated in mode 1 (see
        :func:`search_checked`)."""
        check(self.lib.rpr_set_forced_tail(self.handle, int(mode)), "rpr_set_forced_tail")

    def forced_tail(self) -> int:
        return int(self.lib.rpr_forced_tail(self.handle))

    def set_fork_depths(self, depths: Optional[Sequence[int]]):
        """Explicit fork depths (ascending, at most two; ``[]`` = never fork); ``None`` = choose from the trie statistics."""
        if depths is None:
            check(self.lib.rpr_set_fork_depths(self.handle, -1, None), "rpr_set_fork_depths")
        else:
            arr = (C.c_int32 * max(1, len(depths)))(*[int(d) for d in depths])
            check(self.lib.rpr_set_fork_depths(self.handle, len(depths), arr), "rpr_set_fork_depths")

    def fork_depths(self, model: "DeviceModel", trie: "DeviceTrie", Q: int, B: int, L: int, log_softmax: bool = False) -> List[int]:
        """The fork depths a search of this shape would use (``rpr_fork_depths``)."""
        out = (C.c_int32 * 2)()
        n = int(self.lib.rpr_fork_depths(self.handle, model.handle, trie.handle, Q, B, L,
                                         _lib.FLAG_LOG_SOFTMAX if log_softmax else 0, out))
        if n < 0:
            check(n, "rpr_fork_depths")
        return [int(out[i]) for i in range(n)]

    def last_fork_stats(self) -> List[dict]:
        """Per fork of the last search: depth, queries forced there, queries that walked on (synchronises the device)."""
        d, f, l = (C.c_int32 * 2)(), (C.c_int32 * 2)(), (C.c_int32 * 2)()
        n = int(self.lib.rpr_last_fork_stats(self.handle, d, f, l))
        if n < 0:
            check(n, "rpr_last_fork_stats")
        return [dict(depth=int(d[i]), forced=int(f[i]), left=int(l[i])) for i in range(n)]

    def status_async(self, clear: bool = True):
        """Flags of the work enqueued so far WITHOUT synchronising (``rpr_status_words_async``): returns a
        :class:`StatusTicket` whose ``flags()`` waits only for the copy enqueued here."""
        words = torch.zeros(4, dtype=torch.int32).pin_memory()
        check(self.lib.rpr_status_words_async(self.handle, _stream_ptr(self.device), words.data_ptr(), 1 if clear else 0),
              "rpr_status_words_async")
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return StatusTicket(words, ev)

    def clear_status_async(self):
        check(self.lib.rpr_status_words_async(self.handle, _stream_ptr(self.device), None, 1), "rpr_status_words_async")

    def status(self, clear: bool = True) -> int:
        """Synchronises the current stream and returns the sticky status flags of the work enqueued so far
        (``_lib.STATUS_SATURATED``: an activation left the f16 plane range in f16x2 mode and was clamped — the results
        since the last clear must be recomputed in 'f32' precision, and so after ``_lib.STATUS_SMALL_STREAM``: a row of the
        residual stream under the RMS floor of the f16 planes and the fixed-point row sums; ``_lib.STATUS_EMPTY_QUERY``)."""
        out = C.c_uint32(0)
        check(self.lib.rpr_get_status(self.handle, _stream_ptr(self.device), C.byref(out), 1 if clear else 0), "rpr_get_status")
        flags = int(out.value) | getattr(self, "_kept_status", 0)
        if clear:
            self._kept_status = 0
        return flags

    def keep_status(self, flags: int):
        """Hand flags back that a caller read with ``status(clear=True)`` but does not own (the device words are gone):
        the next ``status()`` reports them again. Used by side passes that must clear the device words around their own
        run (tasks/generation.py ``_per_step_record``) without swallowing another search's unchecked flags."""
        self._kept_status = getattr(self, "_kept_status", 0) | int(flags)

    # -- profiling (bench.py roofline leg) --
    def profile_enable(self, on: bool):
        check(self.lib.rpr_profile_enable(self.handle, 1 if on else 0), "rpr_profile_enable")

    def profile_reset(self):
        check(self.lib.rpr_profile_reset(self.handle), "rpr_profile_reset")

    def profile_get(self) -> Dict[str, dict]:
        out = {}
        for cls, name in enumerate(_lib.KERNEL_CLASS_NAMES):
            st = _lib.KernelStats()
            check(self.lib.rpr_profile_get(self.handle, cls, C.byref(st)), "rpr_profile_get")
            out[name] = dict(total_ms=st.total_ms, launches=int(st.launches), flops=st.flops, bytes=st.bytes)
        return out

    # -- single operators (kernel-level parity tests) --
    def linear(self, A: torch.Tensor, W: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False):
        assert A.is_cuda and W.is_cuda and A.dtype == torch.float32 and W.dtype == torch.float32
        A, W = A.contiguous(), W.contiguous()
        M, K = A.shape
        N = W.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
        res = residual.contiguous() if residual is not None else None
        check(self.lib.rpr_op_linear(self.handle, A.data_ptr(), W.data_ptr(), res.data_ptr() if res is not None else None,
                                     out.data_ptr(), M, N, K, 1 if relu else 0, _stream_ptr(A.device)), "rpr_op_linear")
        return out

    def linear_h2(self, A: torch.Tensor, W: torch.Tensor, mode: int = 0, mfma16: int = 0, relu: bool = False,
                  resid: Optional[torch.Tensor] = None, row_ssq: Optional[torch.Tensor] = None, eps: float = 0.0,
                  m_dev: Optional[torch.Tensor] = None, rm_B: int = 0, split_n: int = 0, out0: Optional[torch.Tensor] = None,
                  out1: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None,
                  out_planes: Optional[torch.Tensor] = None, ssq_out: Optional[torch.Tensor] = None):
        """Test hook (``rpr_op_linear_h2``, modes RPR_LIN_*): one split-precision launch with a search's epilogue, written
        into the caller's buffers (fp32 out0 / out1 / out2, float16 out_planes [2, M, N], int64 ssq_out / row_ssq, int32 m_dev)."""
        assert A.is_cuda and W.is_cuda and A.dtype == torch.float32 and W.dtype == torch.float32 and A.is_contiguous() and W.is_contiguous()
        M, K = A.shape
        p = lambda t: t.data_ptr() if t is not None else None
        check(self.lib.rpr_op_linear_h2(self.handle, A.data_ptr(), W.data_ptr(), M, W.shape[0], K, int(mode), int(mfma16), 1 if relu else 0,
                                        p(resid), p(row_ssq), float(eps), p(m_dev), int(rm_B), int(split_n), p(out0), p(out1), p(out2),
                                        p(out_planes), p(ssq_out), _stream_ptr(A.device)), "rpr_op_linear_h2")

    def linear_bf16(self, A: torch.Tensor, W: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False,
                    n_products: int = 0):
        """The bf16 GEMM kernels of the fine-tune step (rpr_op_linear_bf16). n_products = 0: one product through the step's own
        kernel choice -> [M, N]; n_products >= 1: the grouped weight-gradient launch -> [n_products, M, N] (product i = the
        first M - 256 i rows of A; the rows behind them stay zero)."""
        assert A.is_cuda and W.is_cuda and A.dtype == torch.float32 and W.dtype == torch.float32
        A, W = A.contiguous(), W.contiguous()
        M, K = A.shape
        N = W.shape[0]
        shape = (M, N) if n_products == 0 else (n_products, M, N)
        out = torch.zeros(shape, dtype=torch.float32, device=A.device)
        res = residual.contiguous() if residual is not None else None
        check(self.lib.rpr_op_linear_bf16(self.handle, A.data_ptr(), W.data_ptr(), res.data_ptr() if res is not None else None,
                                          out.data_ptr(), M, N, K, 1 if relu else 0, n_products, _stream_ptr(A.device)),
              "rpr_op_linear_bf16")
        return out

    def rmsnorm(self, x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6):
        x, w = x.contiguous(), w.contiguous()
        out = torch.empty_like(x)
        check(self.lib.rpr_op_rmsnorm(self.handle, x.data_ptr(), w.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                      eps, _stream_ptr(x.device)), "rpr_op_rmsnorm")
        return out

    # -- attention test hooks (rpr_op_*_attn): one launch of a search's attention site into the caller's buffers; every
    #    method returns the name of the kernel the site's planner chose. Tensors are device tensors (None = NULL pointer).
    def _attn_op(self, fn_name: str, op, dev) -> str:
        k = C.c_int32(-1)
        check(getattr(self.lib, fn_name)(self.handle, C.byref(op), C.byref(k), _stream_ptr(dev)), fn_name)
        return self.lib.rpr_attn_kernel_name(int(k.value)).decode()

    def enc_attn(self, qkv, mask, rel_bias, Q, Lq, H, dkv=64, num_buckets=32, max_distance=128, causal=False, mfma=False,
                 offs=None, lens=None, out=None, out_planes=None, plane_stride=0) -> str:
        p = lambda t: t.data_ptr() if t is not None else None
        op = _lib.EncAttnOp(p(qkv), p(mask), p(rel_bias), p(offs), p(lens), p(out), p(out_planes), int(plane_stride),
                            num_buckets, max_distance, Q, Lq, H, dkv, 1 if causal else 0, 1 if mfma else 0)
        return self._attn_op("rpr_op_enc_attn", op, qkv.device)

    def dec_self_attn(self, q, kcache, vcache, strides, anc, rel_bias, Q, B, H, t, dkv=64, num_buckets=32, max_distance=128,
                      nq_dev=None, out=None, out_planes=None, plane_stride=0) -> str:
        """strides = (q_stride, h_stride, pos_stride, slot_stride) in floats; anc: uint16 rows as int16 storage [Q * B, anc_ld]."""
        p = lambda t_: t_.data_ptr() if t_ is not None else None
        op = _lib.DecSelfAttnOp(p(q), p(kcache), p(vcache), p(anc), p(rel_bias), p(nq_dev), p(out), p(out_planes), int(plane_stride),
                                *[int(x) for x in strides], anc.shape[1], num_buckets, max_distance, Q, B, H, t, dkv)
        return self._attn_op("rpr_op_dec_self_attn", op, q.device)

    def cross_attn(self, site, q, xk, xv, xld, mask, Q, B, H, Lq, dkv=64, offs=None, nq_dev=None, out=None, out_planes=None,
                   plane_stride=0) -> str:
        """site: _lib.CROSS_SITE_BLOCK / _STEP / _TAIL."""
        p = lambda t: t.data_ptr() if t is not None else None
        op = _lib.CrossAttnOp(p(q), p(xk), p(xv), p(mask), p(offs), p(nq_dev), p(out), p(out_planes), int(plane_stride),
                              int(site), xld, Q, B, H, Lq, dkv)
        return self._attn_op("rpr_op_cross_attn", op, q.device)

    def tail_self_attn(self, qkv, kcache, vcache, strides, anc, flist, kvq, nseq_dev, rel_bias, nseq_cap, B, H, T, L, dkv=64,
                       num_buckets=32, max_distance=128, out=None, out_planes=None, plane_stride=0) -> str:
        p = lambda t: t.data_ptr() if t is not None else None
        op = _lib.TailSelfAttnOp(p(qkv), p(kcache), p(vcache), p(anc), p(flist), p(kvq), p(nseq_dev), p(rel_bias), p(out), p(out_planes),
                                 int(plane_stride), *[int(x) for x in strides], anc.shape[1], num_buckets, max_distance, nseq_cap,
                                 B, H, T, L, dkv)
        return self._attn_op("rpr_op_tail_self_attn", op, qkv.device)

    # -- the training step's attention (rpr_op_train_*_attn_*): drop = None or (rate, seed, step, site, L)
    @staticmethod
    def _attn_drop(drop):
        if drop is None:
            return _lib.AttnDrop(0, 0, 0.0, 0, 0)
        rate, seed, step, site, L = drop
        return _lib.AttnDrop(int(seed), int(step), float(rate), int(site), int(L))

    def _train_self_attn_op(self, qkv, dO, mask, rel_bias, dqkv, dbias, out, S, Ls, H, dkv, num_buckets, max_distance, causal, drop):
        p = lambda t: t.data_ptr() if t is not None else None
        return _lib.TrainSelfAttnOp(p(qkv), p(dO), p(mask), p(rel_bias), p(dqkv), p(dbias), p(out), self._attn_drop(drop),
                                    num_buckets, max_distance, S, Ls, H, dkv, 1 if causal else 0)

    def train_self_attn_bwd(self, qkv, dO, mask, rel_bias, dqkv, dbias, S, Ls, H, dkv=64, num_buckets=32, max_distance=128,
                            causal=False, drop=None) -> str:
        """dqkv is written, dbias [num_buckets, H] is added to."""
        op = self._train_self_attn_op(qkv, dO, mask, rel_bias, dqkv, dbias, None, S, Ls, H, dkv, num_buckets, max_distance, causal, drop)
        return self._attn_op("rpr_op_train_self_attn_bwd", op, qkv.device)

    def train_self_attn_drop_fwd(self, qkv, mask, rel_bias, out, S, Ls, H, drop, dkv=64, num_buckets=32, max_distance=128,
                                 causal=False) -> str:
        op = self._train_self_attn_op(qkv, None, mask, rel_bias, None, None, out, S, Ls, H, dkv, num_buckets, max_distance, causal, drop)
        return self._attn_op("rpr_op_train_self_attn_drop_fwd", op, qkv.device)

    def _train_cross_attn_op(self, q, dO, xk, xv, xld, mask, dq, dxk, dxv, out, bz, n, Lq, H, dkv, drop):
        p = lambda t: t.data_ptr() if t is not None else None
        return _lib.TrainCrossAttnOp(p(q), p(dO), p(xk), p(xv), p(mask), p(dq), p(dxk), p(dxv), p(out), self._attn_drop(drop),
                                     xld, bz, n, Lq, H, dkv)

    def train_cross_attn_bwd(self, q, dO, xk, xv, xld, mask, dq, dxk, dxv, bz, n, Lq, H, dkv=64, drop=None) -> str:
        """dxk / dxv: rows of xld floats like xk / xv; only the head columns of a row are written."""
        op = self._train_cross_attn_op(q, dO, xk, xv, xld, mask, dq, dxk, dxv, None, bz, n, Lq, H, dkv, drop)
        return self._attn_op("rpr_op_train_cross_attn_bwd", op, q.device)

    def train_cross_attn_drop_fwd(self, q, xk, xv, xld, mask, out, bz, n, Lq, H, drop, dkv=64) -> str:
        op = self._train_cross_attn_op(q, None, xk, xv, xld, mask, None, None, None, out, bz, n, Lq, H, dkv, drop)
        return self._attn_op("rpr_op_train_cross_attn_drop_fwd", op, q.device)

    def train_rows(self, op_name: str, src=(), dst=(), dims=(), f=()):
        """Test hook of the training step's row-wise kernels (``rpr_op_train_rows``): launcher ``op_name`` (a key of
        _lib.TRAIN_ROWS_OPS) on device tensors src / dst (None = NULL) with the integer / float arguments dims / f, each in the
        order include/ripor_hip.h lists for the op."""
        op = _lib.TrainRowsOp()
        dev = None
        for arr, ts in ((op.src, src), (op.dst, dst)):
            assert len(ts) <= len(arr)
            for i, t in enumerate(ts):
                if t is not None:
                    assert t.is_cuda
                    dev = dev or t.device
                    arr[i] = t.data_ptr()
        op.op = _lib.TRAIN_ROWS_OPS[op_name]
        assert len(dims) <= len(op.dims) and len(f) <= len(op.f)
        for i, v in enumerate(dims):
            op.dims[i] = int(v)
        for i, v in enumerate(f):
            op.f[i] = float(v)
        check(self.lib.rpr_op_train_rows(self.handle, C.byref(op), _stream_ptr(dev)), "rpr_op_train_rows " + op_name)


class StatusTicket:
    """Status words of a ctx as of one point of a stream (``Context.status_async``)."""

    def __init__(self, words: torch.Tensor, event):
        self._words, self._event = words, event

    def flags(self) -> int:
        self._event.synchronize()
        w = self._words
        return ((_lib.STATUS_SATURATED if int(w[0]) else 0) | (_lib.STATUS_EMPTY_QUERY if int(w[1]) else 0) |
                (_lib.STATUS_TAIL_LEFTOVER if int(w[2]) else 0) | (_lib.STATUS_SMALL_STREAM if int(w[3]) else 0))


def rel_bucket(rel: int, bidirectional: bool, num_buckets: int = 32, max_distance: int = 128) -> int:
    """Host-only table entry exactly as the library computes it (needs no GPU)."""
    return int(_lib.load().rpr_rel_bucket(rel, 1 if bidirectional else 0, num_buckets, max_distance))


def read_docid_to_smtid(path: str):
    """``docid_to_smtid.json`` -> (docids: list[str] in file order, codes: uint16 ``[N, L]`` without the
    leading -1). Streaming C++ reader (``rpr_d2s_*``); host only, needs no GPU. Replaces the reference's
    ``ujson.load`` + per-doc list slicing (evaluate.py:400-402, 439-446)."""
    lib = _lib.load()
    h = C.c_void_p()
    check(lib.rpr_d2s_open(path.encode(), C.byref(h)), "rpr_d2s_open")
    try:
        N, L, kb = C.c_int64(), C.c_int32(), C.c_int64()
        check(lib.rpr_d2s_dims(h, C.byref(N), C.byref(L), C.byref(kb)), "rpr_d2s_dims")
        codes = np.empty((N.value, L.value), dtype=np.uint16)
        keys = C.create_string_buffer(max(1, kb.value))
        check(lib.rpr_d2s_copy(h, codes.ctypes.data_as(C.c_void_p), keys), "rpr_d2s_copy")
        docids = keys.raw[:kb.value].decode("utf-8").split("\n")
    finally:
        lib.rpr_d2s_close(h)
    assert len(docids) == codes.shape[0], (len(docids), codes.shape)
    return docids, codes


def build_trie_file(codes: np.ndarray, V: int, path: str, docids: Optional[Sequence[str]] = None,
                    source_path: Optional[str] = None) -> None:
    """HOST ONLY (no GPU, no ctx): sort the docid code matrix and write the binary trie cache (``rpr_trie_build_file``),
    optionally with the docid strings and the identity (size, mtime) of the JSON the codes came from."""
    import os
    lib = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    N, L = codes.shape
    keys = "\n".join(docids).encode("utf-8") if docids is not None else b""
    if docids is not None and len(docids) != N:
        raise ValueError("one docid per code row expected")
    size = mtime = 0
    if source_path is not None:
        st = os.stat(source_path)
        size, mtime = st.st_size, st.st_mtime_ns
    check(lib.rpr_trie_build_file(codes.ctypes.data_as(C.c_void_p), N, L, int(V), keys, len(keys), size, mtime,
                                  path.encode()), "rpr_trie_build_file")


def trie_single_frac(codes: np.ndarray, L: Optional[int] = None) -> np.ndarray:
    """HOST ONLY: share of the depth-t trie nodes (t = 0..L) that hold a single distinct L-token sequence
    (``rpr_trie_single_frac``) — the statistic behind the automatic fork depths of the forced-tail search."""
    lib = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    N, Lc = codes.shape
    L = Lc if L is None else int(L)
    out = (C.c_double * (L + 1))()
    check(lib.rpr_trie_single_frac(codes.ctypes.data_as(C.c_void_p), N, Lc, L, out), "rpr_trie_single_frac")
    return np.asarray(list(out), dtype=np.float64)


def trie_extra_mean(codes: np.ndarray, L: Optional[int] = None) -> np.ndarray:
    """``out[t]`` = mean over the depth-t trie nodes of (distinct L-token sequences under the node - 1), host only
    (``rpr_trie_extra_mean``) — the statistic behind the fork depths of a search that forces queries with extras."""
    lib = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    N, Lc = codes.shape
    L = Lc if L is None else int(L)
    out = (C.c_double * (L + 1))()
    check(lib.rpr_trie_extra_mean(codes.ctypes.data_as(C.c_void_p), N, Lc, L, out), "rpr_trie_extra_mean")
    return np.array(out[:], dtype=np.float64)


def plan_forks(single_frac: np.ndarray, extra_mean: np.ndarray, Q: int, B: int, L: int, forced_tail: int = 1,
               tail_extras: int = -1):
    """The fork depths the library derives from the two trie statistics, host only (``rpr_plan_forks``): ``(depths,
    drop_last)``."""
    lib = _lib.load()
    f = (C.c_double * (L + 1))(*[float(x) for x in single_frac[:L + 1]])
    mu = (C.c_double * (L + 1))(*[float(x) for x in extra_mean[:L + 1]])
    depths, drop = (C.c_int32 * 2)(), C.c_int32(0)
    n = int(lib.rpr_plan_forks(f, mu, int(Q), int(B), int(L), int(forced_tail), int(tail_extras), depths, C.byref(drop)))
    if n < 0:
        check(n, "rpr_plan_forks")
    return [int(depths[i]) for i in range(n)], bool(drop.value)


def trie_file_info(path: str) -> dict:
    """Header of a binary trie file (host only): N, L, V, key_bytes, src_size, src_mtime_ns."""
    lib = _lib.load()
    n, l, v, kb, ss, sm = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.rpr_trie_file_info(path.encode(), C.byref(n), C.byref(l), C.byref(v), C.byref(kb), C.byref(ss), C.byref(sm)),
          "rpr_trie_file_info")
    return dict(N=n.value, L=l.value, V=v.value, key_bytes=kb.value, src_size=ss.value, src_mtime_ns=sm.value)


def _ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


class DeviceModel:
    """Binds a ``T5ForDocIDGeneration`` state dict (reference checkpoint key names, SURVEY.md §8
    row a14) to an ``rpr_model``: q/k/v are concatenated, codebooks and cross-attention k/v stacked,
    everything float32 on the device. The feed-forward kind is ``cfg.feed_forward_proj`` where the config object has one
    (``"relu"`` or ``"gated-gelu"``), else what the state dict holds (``wi`` or ``wi_0`` / ``wi_1``); a gated block's two
    input matrices are concatenated like q/k/v (rows 0..d_ff-1 = wi_0, the gate)."""

    def __init__(self, ctx: Context, state_dict: Dict[str, torch.Tensor], cfg):
        self.ctx, self.cfg = ctx, cfg
        dev = ctx.device

        def g(name):
            t = state_dict[name]
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(t)
            return t.to(device=dev, dtype=torch.float32).contiguous()

        L = len(cfg.decoder_vocab_sizes)
        V = int(cfg.decoder_vocab_sizes[0])
        if len(set(cfg.decoder_vocab_sizes)) != 1:
            raise ValueError("not valid decoder_vocab_size")  # reference evaluate.py:433-436
        shared_embeds = bool(cfg.shared_output_input_embeds)
        keep: List[torch.Tensor] = []
        # (checkpoint tensor name, packed device tensor, slice of it or None): how the packed tensors map back to names
        self._names: List[tuple] = []

        def K(t):
            keep.append(t)
            return t

        def N(name, t, sl=None):
            self._names.append((name, t, sl))
            return t

        def attn_qkv(prefix):
            t = K(torch.cat([g(prefix + ".q.weight"), g(prefix + ".k.weight"), g(prefix + ".v.weight")], 0).contiguous())
            n = t.shape[0] // 3
            for j, w in enumerate("qkv"):
                N(f"{prefix}.{w}.weight", t, slice(j * n, (j + 1) * n))
            return t

        has_gate = "encoder.block.0.layer.1.DenseReluDense.wi_0.weight" in state_dict
        kind = getattr(cfg, "feed_forward_proj", "gated-gelu" if has_gate else "relu")
        if kind not in ("relu", "gated-gelu"):
            raise ValueError(f"feed_forward_proj={kind!r} is not supported: the feed-forward block is one of 'relu', 'gated-gelu'")
        self.gated_ff = kind == "gated-gelu"

        def ff_wi(prefix):
            if not self.gated_ff:
                return N(prefix + ".wi.weight", K(g(prefix + ".wi.weight")))
            t = K(torch.cat([g(prefix + ".wi_0.weight"), g(prefix + ".wi_1.weight")], 0).contiguous())
            n = t.shape[0] // 2
            for j in range(2):
                N(f"{prefix}.wi_{j}.weight", t, slice(j * n, (j + 1) * n))
            return t

        ne, nd = cfg.num_layers, cfg.num_decoder_layers
        enc = dict(ln0=[], qkv=[], o=[], ln1=[], wi=[], wo=[])
        for i in range(ne):
            p = f"encoder.block.{i}.layer"
            enc["ln0"].append(N(p + ".0.layer_norm.weight", K(g(p + ".0.layer_norm.weight"))))
            enc["qkv"].append(attn_qkv(p + ".0.SelfAttention"))
            enc["o"].append(N(p + ".0.SelfAttention.o.weight", K(g(p + ".0.SelfAttention.o.weight"))))
            enc["ln1"].append(N(p + ".1.layer_norm.weight", K(g(p + ".1.layer_norm.weight"))))
            enc["wi"].append(ff_wi(p + ".1.DenseReluDense"))
            enc["wo"].append(N(p + ".1.DenseReluDense.wo.weight", K(g(p + ".1.DenseReluDense.wo.weight"))))
        dec = dict(ln0=[], qkv=[], o=[], ln1=[], xq=[], xo=[], ln2=[], wi=[], wo=[])
        xkv = []
        for i in range(nd):
            p = f"decoder.block.{i}.layer"
            dec["ln0"].append(N(p + ".0.layer_norm.weight", K(g(p + ".0.layer_norm.weight"))))
            dec["qkv"].append(attn_qkv(p + ".0.SelfAttention"))
            dec["o"].append(N(p + ".0.SelfAttention.o.weight", K(g(p + ".0.SelfAttention.o.weight"))))
            dec["ln1"].append(N(p + ".1.layer_norm.weight", K(g(p + ".1.layer_norm.weight"))))
            dec["xq"].append(N(p + ".1.EncDecAttention.q.weight", K(g(p + ".1.EncDecAttention.q.weight"))))
            xkv += [g(p + ".1.EncDecAttention.k.weight"), g(p + ".1.EncDecAttention.v.weight")]
            dec["xo"].append(N(p + ".1.EncDecAttention.o.weight", K(g(p + ".1.EncDecAttention.o.weight"))))
            dec["ln2"].append(N(p + ".2.layer_norm.weight", K(g(p + ".2.layer_norm.weight"))))
            dec["wi"].append(ff_wi(p + ".2.DenseReluDense"))
            dec["wo"].append(N(p + ".2.DenseReluDense.wo.weight", K(g(p + ".2.DenseReluDense.wo.weight"))))
        self.shared = N("shared.weight", K(g("shared.weight")))
        self.enc_rel = N("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", K(g("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")))
        self.dec_rel = N("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", K(g("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")))
        self.enc_fln = N("encoder.final_layer_norm.weight", K(g("encoder.final_layer_norm.weight")))
        self.dec_fln = N("decoder.final_layer_norm.weight", K(g("decoder.final_layer_norm.weight")))
        self.start = N("start_token_embed", K(g("start_token_embed").reshape(-1).contiguous()))
        self.in_embeds = K(torch.stack([g(f"list_decoder_embeds.{i}.weight") for i in range(L)], 0).contiguous())
        if shared_embeds:
            self.out_embeds = self.in_embeds
        else:
            self.out_embeds = K(torch.stack([g(f"list_output_embeds.{i}.weight") for i in range(L)], 0).contiguous())
        self.dec_xkv = K(torch.cat(xkv, 0).contiguous())
        inner = cfg.num_heads * cfg.d_kv
        for i in range(nd):
            for j, w in enumerate("kv"):
                N(f"decoder.block.{i}.layer.1.EncDecAttention.{w}.weight", self.dec_xkv,
                  slice((2 * i + j) * inner, (2 * i + j + 1) * inner))
        for i in range(L):
            N(f"list_decoder_embeds.{i}.weight", self.in_embeds, i)
            if not shared_embeds:
                N(f"list_output_embeds.{i}.weight", self.out_embeds, i)
        self._keep = keep
        self._arrays = {}
        d = _lib.ModelDesc()
        d.vocab_size, d.d_model, d.d_kv, d.d_ff = cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff
        d.num_heads, d.num_layers, d.num_decoder_layers = cfg.num_heads, ne, nd
        d.rel_buckets, d.rel_max_distance = cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance
        d.L, d.V = L, V
        d.scaleup_output_hidden = 1 if cfg.scaleup_output_hidden else 0
        d.layer_norm_eps = float(cfg.layer_norm_epsilon)
        d.shared, d.enc_rel_bias, d.dec_rel_bias = self.shared.data_ptr(), self.enc_rel.data_ptr(), self.dec_rel.data_ptr()
        d.enc_final_ln, d.dec_final_ln, d.start_embed = self.enc_fln.data_ptr(), self.dec_fln.data_ptr(), self.start.data_ptr()
        d.in_embeds, d.out_embeds, d.dec_xkv = self.in_embeds.data_ptr(), self.out_embeds.data_ptr(), self.dec_xkv.data_ptr()
        for k, v in enc.items():
            self._arrays["enc_" + k] = _ptr_array(v)
            setattr(d, "enc_" + k, self._arrays["enc_" + k])
        for k, v in dec.items():
            self._arrays["dec_" + k] = _ptr_array(v)
            setattr(d, "dec_" + k, self._arrays["dec_" + k])
        h = C.c_void_p()
        torch.cuda.synchronize(dev)
        ext = _lib.ModelExt(size=C.sizeof(_lib.ModelExt), ff_kind=_lib.FF_GATED_GELU if self.gated_ff else _lib.FF_RELU)
        check(ctx.lib.rpr_load_model_ext(ctx.handle, C.byref(d), C.byref(ext), C.byref(h)), "rpr_load_model_ext")
        self.handle = h
        self._desc = d   # (the per-layer arrays it points to are kept in self._arrays)
        self.L, self.V, self.d_model = L, V, cfg.d_model
        # a weight outside the range of the f16 planes pins the model to the exact-fp32 kernels (rpr_load_model)
        self.f32_only = bool(ctx.lib.rpr_model_f32_only(h))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.ctx.lib.rpr_free_model(self.handle)
                self.handle = None
        except Exception:
            pass

    def named_device_params(self):
        """(checkpoint tensor name, packed device tensor, index / slice of it or None) for every tensor of the model."""
        return list(self._names)

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The model's current device weights under the reference checkpoint's names (after training steps)."""
        out = {}
        for name, t, sl in self._names:
            v = t if sl is None else t[sl]
            out[name] = v.reshape(1, 1, -1).clone() if name == "start_token_embed" else v.clone()
        return out

    def encode(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        dev = self.ctx.device
        ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
        mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
        Q, Lq = ids.shape
        out = torch.empty((Q, Lq, self.d_model), dtype=torch.float32, device=dev)
        check(self.ctx.lib.rpr_encode(self.ctx.handle, self.handle, ids.data_ptr(), mask.data_ptr(), Q, Lq,
                                      out.data_ptr(), _stream_ptr(dev)), "rpr_encode")
        return out


class DeviceTrie:
    """Sorted-code-matrix trie on the device (replaces the reference's dict/CSR structures)."""

    def __init__(self, ctx: Context, handle, L: int, V: int):
        self.ctx, self.handle, self.L, self.V = ctx, handle, L, V
        self.N = int(ctx.lib.rpr_trie_num_rows(handle))
        p = ctx.lib.rpr_trie_perm(handle)
        self.perm = np.ctypeslib.as_array(p, shape=(self.N,))  # view, valid until free

    @classmethod
    def from_codes(cls, ctx: Context, codes: np.ndarray, V: int) -> "DeviceTrie":
        codes = np.ascontiguousarray(codes, dtype=np.uint16)
        N, L = codes.shape
        h = C.c_void_p()
        check(ctx.lib.rpr_build_trie(ctx.handle, codes.ctypes.data_as(C.c_void_p), N, L, V, C.byref(h)), "rpr_build_trie")
        return cls(ctx, h, L, V)

    @classmethod
    def load(cls, ctx: Context, path: str, L: Optional[int] = None, V: Optional[int] = None) -> "DeviceTrie":
        """Load a binary trie file (``rpr_trie_load`` validates it). The depth is the FILE's; ``V`` (the model's decoder
        vocab size) may widen the file's vocab (a cache is built without knowing the model). ``L`` is accepted for
        backward compatibility and only checked against the file."""
        h = C.c_void_p()
        check(ctx.lib.rpr_trie_load(ctx.handle, path.encode(), C.byref(h)), "rpr_trie_load")
        n, fl, fv, kb = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
        check(ctx.lib.rpr_trie_dims(h, C.byref(n), C.byref(fl), C.byref(fv), C.byref(kb)), "rpr_trie_dims")
        try:
            if L is not None and L > fl.value:
                raise RiporHipError(f"{path} holds {fl.value} code columns, {L} requested")
            if V is not None and V != fv.value:
                check(ctx.lib.rpr_trie_set_vocab(h, V), "rpr_trie_set_vocab")
        except Exception:
            ctx.lib.rpr_free_trie(h)
            raise
        t = cls(ctx, h, fl.value, V if V is not None else fv.value)
        t.key_bytes = kb.value
        return t

    def docids(self) -> Optional[List[str]]:
        """docid strings in original row order when the trie came from a file that stores them, else None."""
        kb = getattr(self, "key_bytes", 0)
        if not kb:
            return None
        buf = C.create_string_buffer(kb)
        check(self.ctx.lib.rpr_trie_keys(self.handle, buf), "rpr_trie_keys")
        return buf.raw[:kb].decode("utf-8").split("\n")

    def save(self, path: str):
        check(self.ctx.lib.rpr_trie_save(self.handle, path.encode()), "rpr_trie_save")

    def mask(self, prefix: np.ndarray) -> np.ndarray:
        prefix = np.ascontiguousarray(prefix, dtype=np.int32)
        R, T = prefix.shape
        out = np.zeros((R, self.V), dtype=np.uint8)
        check(self.ctx.lib.rpr_trie_mask(self.ctx.handle, self.handle, prefix.ctypes.data_as(C.c_void_p), R, T,
                                         out.ctypes.data_as(C.c_void_p)), "rpr_trie_mask")
        return out

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.perm = None
                self.ctx.lib.rpr_free_trie(self.handle)
                self.handle = None
        except Exception:
            pass


@dataclass
class SearchResult:
    tokens: torch.Tensor      # int32 [Q, B, L]
    scores: torch.Tensor      # float32 [Q, B]
    row_lo: torch.Tensor      # int64 [Q, B]
    row_hi: torch.Tensor      # int64 [Q, B]
    taps: Optional[dict] = None
    # search(..., margins=True): float64 [Q] pruning margin of every query (include/ripor_hip.h: rpr_search_margins)
    margins: Optional[torch.Tensor] = None
    # search_guarded(..., margin_guard=eps): bool [Q] which queries were searched again in exact fp32 (their rows above are
    # those of the fp32 run), and float64 [rerun.sum()] the fp32 margins of those queries in ascending query order — one
    # still below eps is a near-tie of the reference's own arithmetic, nothing more can be done about it
    rerun: Optional[torch.Tensor] = None
    margins_f32: Optional[torch.Tensor] = None
    # search(..., prefix_lengths=(4, 8)): prefix length p -> the beams of a search of length p (tokens [Q, B, p]; include/ripor_hip.h:
    # rpr_search_prefixes)
    prefixes: Optional[Dict[int, "SearchResult"]] = None


def splice_rows(full, mask, sub):
    """Pure host logic of the near-tie guard: ``full`` is a sequence of arrays with one leading row per query, ``mask`` a
    bool vector over the queries and ``sub`` the same arrays for the masked queries only (ascending query order). Returns the
    arrays with exactly the masked rows replaced — the inputs themselves when nothing is masked, ``sub`` itself when
    everything is; numpy arrays or torch tensors."""
    full, sub = tuple(full), tuple(sub)
    n, q = int(mask.sum()), int(mask.shape[0])
    assert len(full) == len(sub) and all(int(f.shape[0]) == q for f in full) and all(int(x.shape[0]) == n for x in sub)
    if n == 0:
        return full
    if n == q:
        return sub
    out = []
    for f, x in zip(full, sub):
        if isinstance(f, torch.Tensor):
            o = f.clone()
            o[torch.as_tensor(np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask), device=f.device)] = x.to(f.device)
        else:
            o = np.array(f, copy=True)
            o[np.asarray(mask, dtype=bool)] = x
        out.append(o)
    return tuple(out)


def search(model: DeviceModel, trie: DeviceTrie, input_ids: torch.Tensor, attention_mask: torch.Tensor,
           num_beams: int, max_new_tokens: int, apply_log_softmax_for_scores: bool = False,
           use_graph: bool = True, taps: bool = False, margins: bool = False,
           prefix_lengths: Optional[Sequence[int]] = None) -> SearchResult:
    """One call of the hot path: encoder + L fused decode/select steps. Asynchronous on the
    current torch stream; results are device tensors. ``margins``: also the per-query pruning margin
    (``rpr_search_margins``: one more kernel per selection step; tokens, scores and row ranges are the same bits).
    ``prefix_lengths`` (up to three, strictly ascending, each below ``max_new_tokens``): also the beams the search holds
    at those lengths, as ``result.prefixes[p]`` — what a search with ``max_new_tokens=p`` returns (``rpr_search_prefixes``);
    not together with ``taps`` or ``margins``."""
    depths = [int(p) for p in prefix_lengths] if prefix_lengths is not None else []
    if depths and (taps or margins):
        raise ValueError("prefix_lengths cannot be combined with taps or margins")
    ctx = model.ctx
    dev = ctx.device
    ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    Q, Lq = ids.shape
    if not taps and Lq % 8 and Lq < 256:
        # Bucket the padded length to a multiple of 8 (extra columns: id 0, mask 0 — masked keys, identical
        # results). The encoder runs on packed rows, so the padding is free on the device, and a stream of
        # batches with different longest queries reuses a handful of captured hipGraphs instead of one per length.
        pad = min(256, (Lq + 7) // 8 * 8) - Lq
        ids = torch.nn.functional.pad(ids, (0, pad))
        mask = torch.nn.functional.pad(mask, (0, pad))
        Lq += pad
    B, L = int(num_beams), int(max_new_tokens)
    tokens = torch.empty((Q, B, L), dtype=torch.int32, device=dev)
    scores = torch.empty((Q, B), dtype=torch.float32, device=dev)
    lo = torch.empty((Q, B), dtype=torch.int64, device=dev)
    hi = torch.empty((Q, B), dtype=torch.int64, device=dev)
    flags = (_lib.FLAG_LOG_SOFTMAX if apply_log_softmax_for_scores else 0) | (0 if use_graph else _lib.FLAG_NO_GRAPH)
    tap_struct, tap_out = None, None
    if taps:
        tap_out = dict(
            encoder_out=torch.empty((Q, Lq, model.d_model), dtype=torch.float32, device=dev),
            step_logits=torch.empty((L, Q * B, model.V), dtype=torch.float32, device=dev),
            step_scores=torch.empty((L, Q, B), dtype=torch.float64, device=dev),
            step_tokens=torch.empty((L, Q, B), dtype=torch.int32, device=dev),
            step_parent=torch.empty((L, Q, B), dtype=torch.int32, device=dev),
            # bit (beam*V + token) of word [t, q, (beam*V + token) // 64]: token is a trie child of the beam (uint64 bits)
            step_valid=torch.zeros((L, Q, B * model.V // 64), dtype=torch.int64, device=dev))
        tap_struct = _lib.DebugTaps(*[tap_out[k].data_ptr() for k in
                                      ("encoder_out", "step_logits", "step_scores", "step_tokens", "step_parent",
                                       "step_valid")])
    tap_arg = C.byref(tap_struct) if tap_struct is not None else None
    mg = None
    prefixes = None
    if depths:
        # (an invalid list — unsorted, out of range, more than three — is refused by the library before anything is written)
        prefixes = {p: SearchResult(torch.empty((Q, B, max(p, 0)), dtype=torch.int32, device=dev),
                                    torch.empty((Q, B), dtype=torch.float32, device=dev),
                                    torch.empty((Q, B), dtype=torch.int64, device=dev),
                                    torch.empty((Q, B), dtype=torch.int64, device=dev)) for p in depths}
        if len(prefixes) != len(depths):
            raise ValueError("prefix_lengths must be strictly ascending")
        n = len(depths)
        ptrs = lambda f: (C.c_void_p * n)(*[getattr(prefixes[p], f).data_ptr() for p in depths])
        check(ctx.lib.rpr_search_prefixes(ctx.handle, model.handle, trie.handle, ids.data_ptr(), mask.data_ptr(), Q, Lq, B, L,
                                          flags, tokens.data_ptr(), scores.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                          n, (C.c_int32 * n)(*depths), ptrs("tokens"), ptrs("scores"), ptrs("row_lo"),
                                          ptrs("row_hi"), _stream_ptr(dev)), "rpr_search_prefixes")
    elif margins:
        mg = torch.empty((Q,), dtype=torch.float64, device=dev)
        check(ctx.lib.rpr_search_margins(ctx.handle, model.handle, trie.handle, ids.data_ptr(), mask.data_ptr(), Q, Lq, B, L,
                                         flags, tokens.data_ptr(), scores.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                         mg.data_ptr(), tap_arg, _stream_ptr(dev)), "rpr_search_margins")
    else:
        check(ctx.lib.rpr_search(ctx.handle, model.handle, trie.handle, ids.data_ptr(), mask.data_ptr(), Q, Lq, B, L, flags,
                                 tokens.data_ptr(), scores.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                 tap_arg, _stream_ptr(dev)), "rpr_search")
    # ids/mask must stay alive until the async D2D staging copies have been enqueued (they have).
    return SearchResult(tokens, scores, lo, hi, tap_out, margins=mg, prefixes=prefixes)


class GuardedSearch:
    """A search whose device-side guards are checked LATER (no host synchronisation when it is issued).

    ``result()`` waits for the status words copied right behind the search and, if a guard fired, repeats the batch
    synchronously with the safe settings before returning: ``STATUS_TAIL_LEFTOVER`` (optimistic forced-tail mode: a
    query was still unforced at the last fork) -> exact forced-tail mode; ``STATUS_SATURATED`` (an activation left the
    f16 plane range of the split-precision GEMMs) or ``STATUS_SMALL_STREAM`` (a residual row under the RMS floor of that
    path) -> exact fp32 MFMA. ``STATUS_EMPTY_QUERY`` raises ``ValueError``.
    ``repeated`` tells whether the returned result is a second run (its tensors are then new ones).

    ``margin_guard`` (a threshold eps, None = off): the search also computes the per-query pruning margins, and queries
    whose margin is below eps on a ctx that is not already in f32 are searched again as ONE batch in exact fp32; their rows
    replace the split-precision ones (``splice_rows``), and the result carries ``margins``, ``rerun`` and ``margins_f32``."""

    def __init__(self, model, trie, ids, mask, B, L, log_softmax, res, ticket, optimistic=False, margin_guard=None,
                 prefix_lengths=None):
        self._args = (model, trie, ids, mask, B, L, log_softmax)
        self._prefix_lengths = prefix_lengths    # a repeat asks for the same prefix lengths
        self._margin_guard = margin_guard
        # whether the search just issued ran in exact fp32 (the ctx setting, or a model pinned to it): nothing to re-run then
        self._ran_f32 = margin_guard is not None and (
            model.ctx.get_precision() == "f32" or bool(model.ctx.lib.rpr_model_f32_only(model.handle)))
        self._res, self._ticket = res, ticket
        self._optimistic = bool(optimistic)      # this call ran in the optimistic forced-tail mode on the caller's behalf
        self.repeated = False
        self._done = False
        self._error: Optional[BaseException] = None

    def result(self) -> SearchResult:
        if self._done:
            return self._res
        if self._error is not None:   # the guard fired and the repeat failed: the first result is known to be invalid
            raise self._error
        try:
            res = self._result()
        except BaseException as e:
            self._error = e
            raise
        self._done = True
        return res

    def _result(self) -> SearchResult:
        res = self._status_result()
        return res if self._margin_guard is None else self._near_tie_result(res)

    def _near_tie_result(self, res: SearchResult) -> SearchResult:
        model, trie, ids, mask, B, L, log_softmax = self._args
        ctx = model.ctx
        eps = float(self._margin_guard)
        Q = int(res.margins.shape[0])
        rerun = (res.margins < eps).cpu()                 # synchronises the search
        # an exact-fp32 result (the ctx setting, a model pinned to f32, or the saturation guard's repeat) has nothing to re-run
        if self._ran_f32 or not bool(rerun.any()):
            res.rerun = torch.zeros((Q,), dtype=torch.bool)
            res.margins_f32 = torch.empty((0,), dtype=torch.float64, device=res.margins.device)
            self._res = res
            return res
        sel = rerun.to(ids.device)
        saved_mode, saved_prec = ctx.forced_tail(), ctx.get_precision()
        ctx.set_precision("f32")
        if saved_mode == 2:   # the re-run is reported as exact: no query may be left behind at the last fork
            ctx.set_forced_tail(1)
        try:
            ctx.status(clear=True)
            sub = search(model, trie, ids[sel], mask[sel], B, L, apply_log_softmax_for_scores=log_softmax, margins=True)
            st = ctx.status(clear=True)
        finally:
            ctx.set_precision(saved_prec)
            ctx.set_forced_tail(saved_mode)
        if st & _lib.STATUS_TAIL_LEFTOVER:   # cannot happen in the exact mode; never splice unspecified rows in
            raise RuntimeError("near-tie re-run left a query unforced at the last fork")
        tokens, scores, lo, hi = splice_rows((res.tokens, res.scores, res.row_lo, res.row_hi), rerun,
                                             (sub.tokens, sub.scores, sub.row_lo, sub.row_hi))
        self._res = SearchResult(tokens, scores, lo, hi, None, margins=res.margins, rerun=rerun, margins_f32=sub.margins)
        return self._res

    def _status_result(self) -> SearchResult:
        st = self._ticket.flags()
        if st & _lib.STATUS_EMPTY_QUERY:
            raise ValueError("a query has an all-zero attention_mask (no token to attend to)")
        if st & (_lib.STATUS_NEEDS_F32 | _lib.STATUS_TAIL_LEFTOVER):
            model, trie, ids, mask, B, L, log_softmax = self._args
            ctx = model.ctx
            saved_mode, saved_prec = ctx.forced_tail(), ctx.get_precision()
            if (st & _lib.STATUS_NEEDS_F32) and saved_prec != "f32":
                import warnings
                warnings.warn(("activation outside the f16 plane range" if st & _lib.STATUS_SATURATED else
                               "residual stream under the RMS floor") + " of the split-precision GEMMs: repeating this batch "
                              "with exact fp32 MFMA (RPR_PRECISION=f32 avoids the retry)")
                ctx.set_precision("f32")
                self._ran_f32 = True
            if saved_mode == 2:
                ctx.set_forced_tail(1)
            if st & _lib.STATUS_TAIL_LEFTOVER:
                _note_optimistic_outcome(ctx, leftover=True)
            try:
                ctx.status(clear=True)
                self._res = search(model, trie, ids, mask, B, L, apply_log_softmax_for_scores=log_softmax,
                                   margins=self._margin_guard is not None, prefix_lengths=self._prefix_lengths)
                ctx.status(clear=True)
            finally:
                ctx.set_precision(saved_prec)
                ctx.set_forced_tail(saved_mode)
            self.repeated = True
        elif self._optimistic:
            _note_optimistic_outcome(self._args[0].ctx, leftover=False)
        return self._res


# Back-off of the optimistic forced-tail mode (search_guarded). The optimistic mode bets that the last fork leaves no query
# behind; when it loses, the batch is searched twice. On a trie whose popular prefixes stay dense for longer than its node
# statistics suggest (real residual-quantiser codes may) the bet would be lost batch after batch: after two lost bets in a row
# the ctx runs the exact mode for the next OPTIMISTIC_BACKOFF calls, then tries again.
OPTIMISTIC_BACKOFF = 20


def _note_optimistic_outcome(ctx: Context, leftover: bool) -> None:
    if leftover:
        ctx._leftover_streak = getattr(ctx, "_leftover_streak", 0) + 1
        if ctx._leftover_streak >= 2:
            ctx._exact_calls_left = OPTIMISTIC_BACKOFF
    else:
        ctx._leftover_streak = 0


def _optimistic_allowed(ctx: Context) -> bool:
    left = getattr(ctx, "_exact_calls_left", 0)
    if left > 0:
        ctx._exact_calls_left = left - 1
        if ctx._exact_calls_left == 0:
            ctx._leftover_streak = 1      # one more lost bet after the pause and the pause starts again
        return False
    return True


def search_guarded(model: DeviceModel, trie: DeviceTrie, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                   num_beams: int, max_new_tokens: int, apply_log_softmax_for_scores: bool = False,
                   optimistic: Optional[bool] = None, margin_guard: Optional[float] = None,
                   prefix_lengths: Optional[Sequence[int]] = None) -> GuardedSearch:
    """``search`` plus the status guards, checked when ``result()`` is called (see :class:`GuardedSearch`). With
    ``optimistic`` (default: on unless ``RPR_OPTIMISTIC_TAIL=0``) a ctx in the exact forced-tail mode runs this call in
    the optimistic mode — the last, almost always empty, step-by-step stage is not enqueued — and the guard repeats the
    batch exactly in the rare case a query needed it. ``margin_guard`` = eps (None: off, the same calls and the same bits
    as before): the near-tie guard of :class:`GuardedSearch`; 1e-3, the project's tolerance for cumulative scores at the
    pruning boundary, is the suggested value. ``prefix_lengths``: as in ``search``, passed on to a repeat as well; not
    together with ``margin_guard`` (margins are not computed for the shorter lengths)."""
    import os
    if prefix_lengths is not None:
        prefix_lengths = tuple(int(p) for p in prefix_lengths) or None
    if prefix_lengths and margin_guard is not None:
        raise ValueError("prefix_lengths cannot be combined with margin_guard")
    ctx = model.ctx
    if optimistic is None:
        optimistic = os.environ.get("RPR_OPTIMISTIC_TAIL", "1") != "0"
    mode = ctx.forced_tail()
    ctx.clear_status_async()
    went_optimistic = bool(optimistic and mode == 1 and _optimistic_allowed(ctx))
    if went_optimistic:
        ctx.set_forced_tail(2)
    try:
        res = search(model, trie, input_ids, attention_mask, num_beams, max_new_tokens,
                     apply_log_softmax_for_scores=apply_log_softmax_for_scores, margins=margin_guard is not None,
                     prefix_lengths=prefix_lengths)
    finally:
        ctx.set_forced_tail(mode)
    ticket = ctx.status_async(clear=True)
    return GuardedSearch(model, trie, input_ids, attention_mask, int(num_beams), int(max_new_tokens),
                         bool(apply_log_softmax_for_scores), res, ticket, optimistic=went_optimistic, margin_guard=margin_guard,
                         prefix_lengths=prefix_lengths)


def lngknp_forward(model: DeviceModel, input_ids: torch.Tensor, attention_mask: torch.Tensor, doc_codes: torch.Tensor,
                   teacher_pos: Optional[torch.Tensor] = None, teacher_neg: Optional[torch.Tensor] = None,
                   prefix_lens: Optional[Sequence[int]] = None):
    """Forward of the prefix-oriented ranking fine-tune step (``rpr_lngknp_forward``; reference
    T5SeqAQEncoderForLngKnpMarginMSE.forward, modeling/t5_generative_retriever.py:902-966).

    doc_codes ``[bz, n_docs, L]`` (positive first); teacher_pos / teacher_neg ``[n_prefix, bz]`` aligned with
    ``prefix_lens``. Returns ``(losses float32 [n_prefix] or None, position_scores float32 [bz, n_docs, L])``,
    device tensors, asynchronous on the current stream."""
    ctx = model.ctx
    dev = ctx.device
    ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    codes = doc_codes.to(device=dev, dtype=torch.int32).contiguous()
    bz, Lq = ids.shape
    _, n_docs, L = codes.shape
    if Lq % 8 and Lq < 256:   # same bucketing as search(): masked padding columns, identical results
        pad = min(256, (Lq + 7) // 8 * 8) - Lq
        ids = torch.nn.functional.pad(ids, (0, pad)); mask = torch.nn.functional.pad(mask, (0, pad)); Lq += pad
    pos_scores = torch.empty((bz, n_docs, L), dtype=torch.float32, device=dev)
    n_prefix = 0 if prefix_lens is None else len(prefix_lens)
    losses = tp = tn = pl = None
    if n_prefix:
        tp = teacher_pos.to(device=dev, dtype=torch.float32).contiguous()
        tn = teacher_neg.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(tp.shape) == (n_prefix, bz) and tuple(tn.shape) == (n_prefix, bz)
        pl = torch.tensor(list(prefix_lens), dtype=torch.int32, device=dev)
        losses = torch.empty((n_prefix,), dtype=torch.float32, device=dev)
    check(ctx.lib.rpr_lngknp_forward(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq, codes.data_ptr(),
                                     n_docs, L, tp.data_ptr() if n_prefix else None, tn.data_ptr() if n_prefix else None,
                                     pl.data_ptr() if n_prefix else None, n_prefix,
                                     losses.data_ptr() if n_prefix else None, pos_scores.data_ptr(), _stream_ptr(dev)),
          "rpr_lngknp_forward")
    return losses, pos_scores


# ---- training step of the ranking fine-tune: flat gradient / optimizer buffers -----------------------
class TrainState:
    """Flat fp32 buffers of one model replica: gradients and the two AdamW moments, laid out as ``rpr_param_info``
    says (the tensors of ``DeviceModel`` in a fixed order). ``grads`` is what data-parallel ranks all-reduce.

    ``dropout_rate`` / ``dropout_seed``: the dropout the backward entry points apply (``rpr_set_train_dropout``; 0 = off, the
    default). The mask is a stateless function of (seed, global step, site, coordinates): the global step is ``step`` — the
    optimizer steps taken so far, restored with a checkpoint — unless a call names another, so a resumed run draws the masks
    it would have drawn and no RNG state is kept anywhere."""

    def __init__(self, model: DeviceModel, dropout_rate: float = 0.0, dropout_seed: int = 0):
        self.model = model
        self.set_dropout(dropout_rate, dropout_seed)
        lib, h = model.ctx.lib, model.handle
        self.total = int(lib.rpr_param_total(h))
        n = int(lib.rpr_param_count(h))
        self.layout = []   # (device pointer, numel, offset)
        for i in range(n):
            p, ne, off = C.c_void_p(), C.c_int64(), C.c_int64()
            check(lib.rpr_param_info(h, i, C.byref(p), C.byref(ne), C.byref(off)), "rpr_param_info")
            self.layout.append((int(p.value), int(ne.value), int(off.value)))
        dev = model.ctx.device
        self.grads = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.step = 0
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)

    def set_dropout(self, rate: float, seed: int = 0):
        if not 0.0 <= float(rate) < 1.0:
            raise ValueError(f"dropout rate {rate!r} outside [0, 1)")
        self.dropout_rate, self.dropout_seed = float(rate), int(seed) & (2 ** 64 - 1)

    def apply_dropout(self, global_step: Optional[int] = None):
        """Tell the context what the next backward call applies: always called by the backward wrappers, so a state at rate 0
        also switches off what another state of the same context had set."""
        ctx = self.model.ctx
        step = self.step if global_step is None else int(global_step)
        check(ctx.lib.rpr_set_train_dropout(ctx.handle, self.dropout_rate, self.dropout_seed, step), "rpr_set_train_dropout")

    def named_grads(self) -> Dict[str, torch.Tensor]:
        """Gradients under the reference checkpoint's tensor names (q/k/v, the cross k/v and the codebooks un-stacked)."""
        out = {}
        by_ptr = {ptr: (ne, off) for ptr, ne, off in self.layout}
        for name, t, sl in self.model.named_device_params():
            ne, off = by_ptr[t.data_ptr()]
            g = self.grads[off:off + ne].view(t.shape)
            out[name] = g[sl] if sl is not None else g
        return out


class GradExchange:
    """Data-parallel gradient exchange overlapped with the backward pass (the reference wraps the model in
    DistributedDataParallel, tasks/trainer.py:486: bucketed all-reduce running under ``loss.backward()``).

    ``rpr_lngknp_backward_buckets`` hands the flat gradient buffer over in buckets (one per transformer layer in the order
    the backward finishes them, then one for the embeddings / codebooks / cross K/V / norms in front of the first layer):
    for each, ``on_bucket(offset, numel)`` enqueues an asynchronous all-reduce of that slice on a communication stream
    that already waits for the slice's producers. ``finish()`` joins the stream and divides by the world size (DDP's
    averaging). RCCL ("nccl" backend) on GPUs: a bucket is 28-38 MB for t5-base — large messages, as the per-link-bound
    ring on the point-to-point xGMI mesh wants; any torch.distributed backend works (the CPU tests use gloo).
    With one rank (or no process group) nothing is enqueued."""

    def __init__(self, grads: torch.Tensor, dry_run: bool = False, mode: Optional[str] = None):
        """``dry_run`` (tests, one rank): take the buckets and touch each slice on the communication stream instead of
        all-reducing it — the hand-off (callback order, stream dependencies, coverage) without a process group.

        ``mode`` (default: ``RPR_GRAD_EXCHANGE`` or "allreduce"): "allreduce" = one ``all_reduce`` per bucket, the
        algorithm is RCCL's choice; "mesh" = the exchange SURVEY §8 f4 asks for on the point-to-point xGMI mesh: every
        rank owns 1/W of a bucket, receives that shard from all peers at once over the W-1 direct links
        (``all_to_all_single``), sums the W copies in rank order (every rank adds in the same order: the reduced shard has
        one value), and the shards are gathered back (``all_gather_into_tensor``) — reduce-scatter + all-gather in two
        single-hop steps instead of a ring of 2(W-1) per-link-bound steps. Never timed on hardware (no multi-GPU box)."""
        import os
        import torch.distributed as dist
        self.grads = grads
        self.mode = (mode or os.environ.get("RPR_GRAD_EXCHANGE", "allreduce")).lower()
        if self.mode not in ("allreduce", "mesh"):
            raise ValueError(f"unknown gradient exchange mode {self.mode!r} (allreduce | mesh)")
        self._scratch = {}                   # mesh mode: send / receive buffers per padded bucket size
        self.dry_run = bool(dry_run)
        self.active = self.dry_run or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        self.world = dist.get_world_size() if (self.active and not self.dry_run) else 1
        self.stream = torch.cuda.Stream(grads.device) if (self.active and grads.is_cuda) else None
        self.works: List = []
        self.buckets: List[tuple] = []
        self.history: List[tuple] = []       # buckets of the last finished exchange, in hand-over order
        self.error: Optional[BaseException] = None   # first exception raised inside the ctypes callback
        self._cb = _lib.GRAD_BUCKET_CB(self._on_bucket_c)

    def _on_bucket_c(self, _user, offset, numel):
        # ctypes prints and swallows an exception raised inside a callback: the C side would carry on, finish()'s coverage
        # check would pass and AdamW would run on a bucket that was never reduced. Keep the first error; lngknp_backward /
        # finish() re-raise it, and nothing is enqueued after it.
        if self.error is not None:
            return
        try:
            self.on_bucket(int(offset), int(numel))
        except BaseException as e:   # noqa: BLE001 - must not escape into ctypes
            self.error = e

    def on_bucket(self, offset: int, numel: int):
        if not self.active or numel <= 0:
            self.buckets.append((offset, numel))
            return
        sl = self.grads[offset:offset + numel]
        if self.dry_run:
            if self.stream is not None:
                with torch.cuda.stream(self.stream):
                    sl.mul_(1.0)          # reads and rewrites the bucket on the communication stream
        elif self.stream is not None:
            with torch.cuda.stream(self.stream):
                self._exchange(sl)
        else:
            self._exchange(sl)
        self.buckets.append((offset, numel))   # recorded only once its collective has been enqueued

    def raise_pending(self):
        """Re-raise an exception caught inside the bucket callback (and forget the half-done exchange)."""
        if self.error is not None:
            e, self.error = self.error, None
            for w in self.works:   # collectives already in flight must not outlive the buffers they reduce
                try:
                    w.wait()
                except Exception:
                    pass
            if self.stream is not None:
                torch.cuda.current_stream(self.grads.device).wait_stream(self.stream)
            self.works, self.buckets = [], []
            raise RiporHipError(f"gradient exchange failed inside the bucket callback: {e!r}") from e

    def _exchange(self, sl: torch.Tensor):
        import torch.distributed as dist
        if self.mode == "allreduce":
            self.works.append(dist.all_reduce(sl, op=dist.ReduceOp.SUM, async_op=True))
            return
        W, n = self.world, sl.numel()
        per = (n + W - 1) // W
        if per not in self._scratch:         # a handful of distinct bucket sizes (decoder layer, encoder layer, the rest)
            self._scratch[per] = (torch.zeros(W * per, dtype=sl.dtype, device=sl.device),
                                  torch.empty(W * per, dtype=sl.dtype, device=sl.device),
                                  torch.empty(W * per, dtype=sl.dtype, device=sl.device))
        send, recv, full = self._scratch[per]
        send[:n].copy_(sl)                   # the tail of the last shard stays zero
        dist.all_to_all_single(recv, send, async_op=True).wait()     # recv[i] = rank i's copy of MY shard
        shard = recv.view(W, per)[0].clone()
        for i in range(1, W):                # fixed order: bitwise the same sum on every rank for its shard
            shard += recv.view(W, per)[i]
        dist.all_gather_into_tensor(full, shard, async_op=True).wait()
        sl.copy_(full[:n])

    def comm_stream_ptr(self):
        return C.c_void_p(self.stream.cuda_stream) if self.stream is not None else None

    def callback(self):
        return self._cb if self.active else C.cast(None, _lib.GRAD_BUCKET_CB)

    def finish(self):
        """Join the exchange (the current stream waits for every bucket) and average."""
        self.raise_pending()
        for w in self.works:
            w.wait()
        if self.stream is not None:
            torch.cuda.current_stream(self.grads.device).wait_stream(self.stream)
        covered = sum(n for _, n in self.buckets)
        if self.active:
            assert covered == self.grads.numel(), (covered, self.grads.numel())   # every element exchanged exactly once
            if self.world > 1:
                self.grads.div_(self.world)
        self.history = list(self.buckets)
        self.works, self.buckets = [], []


def lngknp_backward(model: DeviceModel, state: TrainState, input_ids, attention_mask, doc_codes, teacher_pos, teacher_neg,
                    prefix_lens: Sequence[int], exchange: Optional[GradExchange] = None,
                    global_step: Optional[int] = None) -> torch.Tensor:
    """Forward + backward of the sum of the margin-MSE losses (``rpr_lngknp_backward``): fills ``state.grads`` and
    returns the losses ``[n_prefix]`` (device tensor). Asynchronous on the current stream. With ``exchange`` the
    gradient all-reduce of every bucket is enqueued while the backward is still running (``GradExchange``); the caller
    then calls ``exchange.finish()`` before the optimizer step. Dropout: what ``state`` says (``TrainState.set_dropout``) at
    ``global_step`` (default: ``state.step``)."""
    ctx = model.ctx
    state.apply_dropout(global_step)
    dev = ctx.device
    ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    codes = doc_codes.to(device=dev, dtype=torch.int32).contiguous()
    bz, Lq = ids.shape
    assert codes.shape[0] == bz and codes.shape[1] == 2
    L = codes.shape[2]
    n_prefix = len(prefix_lens)
    tp = teacher_pos.to(device=dev, dtype=torch.float32).contiguous()
    tn = teacher_neg.to(device=dev, dtype=torch.float32).contiguous()
    assert tuple(tp.shape) == (n_prefix, bz) and tuple(tn.shape) == (n_prefix, bz)
    pl = torch.tensor(list(prefix_lens), dtype=torch.int32, device=dev)
    losses = torch.empty((n_prefix,), dtype=torch.float32, device=dev)
    if exchange is not None and exchange.active:
        check(ctx.lib.rpr_lngknp_backward_buckets(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq,
                                                  codes.data_ptr(), L, tp.data_ptr(), tn.data_ptr(), pl.data_ptr(), n_prefix,
                                                  losses.data_ptr(), state.grads.data_ptr(), _stream_ptr(dev),
                                                  exchange.comm_stream_ptr(), exchange.callback(), None),
              "rpr_lngknp_backward_buckets")
        exchange.raise_pending()
    else:
        check(ctx.lib.rpr_lngknp_backward(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq, codes.data_ptr(), L,
                                          tp.data_ptr(), tn.data_ptr(), pl.data_ptr(), n_prefix, losses.data_ptr(),
                                          state.grads.data_ptr(), _stream_ptr(dev)), "rpr_lngknp_backward")
    return losses


# ---- seq2seq docid cross-entropy step (loss_type t5seq_aq_encoder_seq2seq; reference T5SeqAQEncoderForSeq2Seq) -----------
def _s2s_args(model: DeviceModel, input_ids, attention_mask, labels):
    dev = model.ctx.device
    ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    lab = labels.to(device=dev, dtype=torch.int32).contiguous()
    bz, Lq = ids.shape
    if lab.dim() != 2 or lab.shape[0] != bz:
        raise ValueError(f"labels must be [bz, L] with bz = {bz}, got {tuple(lab.shape)}")
    if Lq > 256:
        raise ValueError(f"queries of {Lq} tokens: the training passes take at most 256 encoder positions (use max_length <= 256)")
    return ids, mask, lab, bz, Lq, int(lab.shape[1])


def seq2seq_forward(model: DeviceModel, input_ids: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor):
    """Forward of the seq2seq docid step (``rpr_seq2seq_forward``): teacher-forced decoder over ``[-1, labels[:, :-1]]``,
    per-position codebook logits, cross-entropy. Returns ``(loss float32 [1], label_logprobs float32 [bz, L])``, device
    tensors, asynchronous on the current stream (after the host-side label check, which synchronises it)."""
    ctx = model.ctx
    ids, mask, lab, bz, Lq, L = _s2s_args(model, input_ids, attention_mask, labels)
    loss = torch.empty((1,), dtype=torch.float32, device=ctx.device)
    lp = torch.empty((bz, L), dtype=torch.float32, device=ctx.device)
    check(ctx.lib.rpr_seq2seq_forward(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq, lab.data_ptr(), L,
                                      loss.data_ptr(), lp.data_ptr(), _stream_ptr(ctx.device)), "rpr_seq2seq_forward")
    return loss, lp


def seq2seq_backward(model: DeviceModel, state: TrainState, input_ids, attention_mask, labels,
                     exchange: Optional[GradExchange] = None, global_step: Optional[int] = None) -> torch.Tensor:
    """Forward + backward of the seq2seq cross-entropy (``rpr_seq2seq_backward``): fills ``state.grads`` and returns the loss
    ``[1]`` (device tensor). With ``exchange`` the gradient buckets are handed over, and dropout is applied, as in
    :func:`lngknp_backward`."""
    ctx = model.ctx
    state.apply_dropout(global_step)
    ids, mask, lab, bz, Lq, L = _s2s_args(model, input_ids, attention_mask, labels)
    loss = torch.empty((1,), dtype=torch.float32, device=ctx.device)
    if exchange is not None and exchange.active:
        check(ctx.lib.rpr_seq2seq_backward_buckets(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq, lab.data_ptr(), L,
                                                   loss.data_ptr(), state.grads.data_ptr(), _stream_ptr(ctx.device),
                                                   exchange.comm_stream_ptr(), exchange.callback(), None),
              "rpr_seq2seq_backward_buckets")
        exchange.raise_pending()
    else:
        check(ctx.lib.rpr_seq2seq_backward(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq, lab.data_ptr(), L,
                                           loss.data_ptr(), state.grads.data_ptr(), _stream_ptr(ctx.device)), "rpr_seq2seq_backward")
    return loss


def seq2seq_train_step(model: DeviceModel, state: TrainState, input_ids, attention_mask, labels, lr: float, betas=(0.9, 0.999),
                       eps: float = 1e-8, weight_decay: float = 0.0, max_grad_norm: float = 1.0,
                       dropout_rate: Optional[float] = None, dropout_seed: Optional[int] = None,
                       global_step: Optional[int] = None) -> torch.Tensor:
    """:func:`train_step` for the seq2seq cross-entropy: backward with the gradient exchange (bucketed and overlapped unless
    ``RPR_GRAD_OVERLAP=0``), clip_grad_norm_, AdamW. Returns the loss ``[1]`` before the update."""
    import os
    if dropout_rate is not None:
        state.set_dropout(dropout_rate, state.dropout_seed if dropout_seed is None else dropout_seed)
    if os.environ.get("RPR_GRAD_OVERLAP", "1") == "0":
        loss = seq2seq_backward(model, state, input_ids, attention_mask, labels, global_step=global_step)
        allreduce_grads(state)
    else:
        ex = getattr(state, "_exchange", None)
        if ex is None or ex.grads is not state.grads:
            ex = state._exchange = GradExchange(state.grads)
        loss = seq2seq_backward(model, state, input_ids, attention_mask, labels, exchange=ex, global_step=global_step)
        ex.finish()
    adamw_step(model, state, lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    return loss


# ---- dense first-stage step (loss_type t5seq_pretrain_margin_mse; reference T5SeqPretrainEncoder, decoder length 1) --------
def _dense_args(model: DeviceModel, input_ids, attention_mask, teacher_pos, teacher_neg):
    dev = model.ctx.device
    ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    if ids.dim() != 3 or ids.shape[0] != 3 or tuple(mask.shape) != tuple(ids.shape):
        raise ValueError(f"input_ids and attention_mask must be [3, bz, Lt] (queries, positive documents, negative documents), "
                         f"got {tuple(ids.shape)} and {tuple(mask.shape)}")
    _, bz, Lt = ids.shape
    if Lt > 256:
        raise ValueError(f"sequences of {Lt} tokens: the training passes take at most 256 encoder positions (use max_length <= 256)")
    tp = teacher_pos.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    tn = teacher_neg.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    if tp.numel() != bz or tn.numel() != bz:
        raise ValueError(f"teacher scores must be [bz] with bz = {bz}, got {tuple(teacher_pos.shape)} and {tuple(teacher_neg.shape)}")
    return ids, mask, tp, tn, int(bz), int(Lt)


def dense_mse_forward(model: DeviceModel, input_ids, attention_mask, teacher_pos, teacher_neg):
    """Forward of the dense first-stage step (``rpr_dense_mse_forward``): ``input_ids`` / ``attention_mask`` ``[3, bz, Lt]`` hold
    the queries, the positive and the negative documents padded to one length. Returns ``(loss [1], scores [bz, 2], reps
    [3 * bz, d_model])``, float32 device tensors, asynchronous on the current stream; evaluation mode."""
    ctx = model.ctx
    ids, mask, tp, tn, bz, Lt = _dense_args(model, input_ids, attention_mask, teacher_pos, teacher_neg)
    loss = torch.empty((1,), dtype=torch.float32, device=ctx.device)
    scores = torch.empty((bz, 2), dtype=torch.float32, device=ctx.device)
    reps = torch.empty((3 * bz, model.d_model), dtype=torch.float32, device=ctx.device)
    check(ctx.lib.rpr_dense_mse_forward(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lt, tp.data_ptr(), tn.data_ptr(),
                                        loss.data_ptr(), scores.data_ptr(), reps.data_ptr(), _stream_ptr(ctx.device)),
          "rpr_dense_mse_forward")
    return loss, scores, reps


def dense_mse_backward(model: DeviceModel, state: TrainState, input_ids, attention_mask, teacher_pos, teacher_neg,
                       exchange: Optional[GradExchange] = None, global_step: Optional[int] = None) -> torch.Tensor:
    """Forward + backward of the dense margin-MSE (``rpr_dense_mse_backward``): fills ``state.grads`` (the codebooks get exactly
    zero) and returns the loss ``[1]`` (device tensor). ``exchange`` and dropout as in :func:`lngknp_backward`."""
    ctx = model.ctx
    state.apply_dropout(global_step)
    ids, mask, tp, tn, bz, Lt = _dense_args(model, input_ids, attention_mask, teacher_pos, teacher_neg)
    loss = torch.empty((1,), dtype=torch.float32, device=ctx.device)
    if exchange is not None and exchange.active:
        check(ctx.lib.rpr_dense_mse_backward_buckets(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lt, tp.data_ptr(),
                                                     tn.data_ptr(), loss.data_ptr(), state.grads.data_ptr(), _stream_ptr(ctx.device),
                                                     exchange.comm_stream_ptr(), exchange.callback(), None),
              "rpr_dense_mse_backward_buckets")
        exchange.raise_pending()
    else:
        check(ctx.lib.rpr_dense_mse_backward(ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lt, tp.data_ptr(),
                                             tn.data_ptr(), loss.data_ptr(), state.grads.data_ptr(), _stream_ptr(ctx.device)),
              "rpr_dense_mse_backward")
    return loss


def dense_mse_train_step(model: DeviceModel, state: TrainState, input_ids, attention_mask, teacher_pos, teacher_neg, lr: float,
                         betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, max_grad_norm: float = 1.0,
                         dropout_rate: Optional[float] = None, dropout_seed: Optional[int] = None,
                         global_step: Optional[int] = None) -> torch.Tensor:
    """:func:`train_step` for the dense margin-MSE: backward with the gradient exchange (bucketed and overlapped unless
    ``RPR_GRAD_OVERLAP=0``), clip_grad_norm_, AdamW. Returns the loss ``[1]`` before the update."""
    import os
    if dropout_rate is not None:
        state.set_dropout(dropout_rate, state.dropout_seed if dropout_seed is None else dropout_seed)
    if os.environ.get("RPR_GRAD_OVERLAP", "1") == "0":
        loss = dense_mse_backward(model, state, input_ids, attention_mask, teacher_pos, teacher_neg, global_step=global_step)
        allreduce_grads(state)
    else:
        ex = getattr(state, "_exchange", None)
        if ex is None or ex.grads is not state.grads:
            ex = state._exchange = GradExchange(state.grads)
        loss = dense_mse_backward(model, state, input_ids, attention_mask, teacher_pos, teacher_neg, exchange=ex, global_step=global_step)
        ex.finish()
    adamw_step(model, state, lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    return loss


def allreduce_grads(state: TrainState, bucket_elems: int = 64 << 20) -> None:
    """Serial data-parallel gradient exchange (``RPR_GRAD_OVERLAP=0``; the default is :class:`GradExchange`, overlapped
    with the backward pass): sum ``state.grads`` over the ranks in a few large chunks after the backward and divide by
    the world size (DDP's gradient averaging). RCCL ("nccl" backend) on GPUs; any torch.distributed backend works. The
    MI355X xGMI mesh is point-to-point, so few large messages are what RCCL's ring needs: 256 MB chunks by default."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    world = dist.get_world_size()
    g = state.grads
    for s in range(0, g.numel(), bucket_elems):
        dist.all_reduce(g[s:s + bucket_elems], op=dist.ReduceOp.SUM)
    g.div_(world)


def allreduce_mode() -> str:
    import os
    if os.environ.get("RPR_GRAD_OVERLAP", "1") == "0":
        return "serial"
    how = "all_to_all + all_gather per bucket (mesh)" if os.environ.get("RPR_GRAD_EXCHANGE", "allreduce").lower() == "mesh" else "all_reduce per bucket"
    return f"bucketed, overlapped with the backward pass, {how}"


def train_step(model: DeviceModel, state: TrainState, input_ids, attention_mask, doc_codes, teacher_pos, teacher_neg,
               prefix_lens: Sequence[int], lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
               max_grad_norm: float = 1.0, dropout_rate: Optional[float] = None, dropout_seed: Optional[int] = None,
               global_step: Optional[int] = None) -> torch.Tensor:
    """One optimisation step as the reference's trainer performs it (tasks/trainer.py:203-275 + HF Trainer defaults):
    forward + backward, gradient all-reduce across the data-parallel ranks — bucketed and overlapped with the backward
    (``RPR_GRAD_OVERLAP=0``: one serial pass afterwards) —, clip_grad_norm_, AdamW. Returns the losses before the update.
    ``dropout_rate`` / ``dropout_seed`` (default: what ``state`` holds, off unless set) and ``global_step`` (default:
    ``state.step``, the optimizer steps taken so far) select the dropout masks of this step (``rpr_set_train_dropout``)."""
    import os
    if dropout_rate is not None:
        state.set_dropout(dropout_rate, state.dropout_seed if dropout_seed is None else dropout_seed)
    if os.environ.get("RPR_GRAD_OVERLAP", "1") == "0":
        losses = lngknp_backward(model, state, input_ids, attention_mask, doc_codes, teacher_pos, teacher_neg, prefix_lens,
                                 global_step=global_step)
        allreduce_grads(state)
    else:
        ex = getattr(state, "_exchange", None)
        if ex is None or ex.grads is not state.grads:
            ex = state._exchange = GradExchange(state.grads)
        losses = lngknp_backward(model, state, input_ids, attention_mask, doc_codes, teacher_pos, teacher_neg, prefix_lens,
                                 exchange=ex, global_step=global_step)
        ex.finish()
    adamw_step(model, state, lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    return losses


def adamw_step(model: DeviceModel, state: TrainState, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 0.0, max_grad_norm: float = 1.0) -> None:
    """``clip_grad_norm_(max_grad_norm)`` + ``torch.optim.AdamW`` on the model's device tensors, in place
    (``rpr_adamw_step``); ``state.grad_norm`` receives the pre-clip global norm."""
    ctx = model.ctx
    state.step += 1
    check(ctx.lib.rpr_adamw_step(ctx.handle, model.handle, state.grads.data_ptr(), state.exp_avg.data_ptr(),
                                 state.exp_avg_sq.data_ptr(), state.step, lr, betas[0], betas[1], eps, weight_decay,
                                 max_grad_norm, state.grad_norm.data_ptr(), _stream_ptr(ctx.device)), "rpr_adamw_step")


# ---- residual quantization: docid creation (rpr_rq_train / rpr_rq_encode; DESIGN.md "Residual quantization") ----
RQ_NITER, RQ_SEED, RQ_MAX_POINTS_PER_CENTROID = 25, 1234, 256   # faiss's k-means defaults


def rq_training_plan(N: int, M: int, K: int, seed: int = RQ_SEED):
    """HOST ONLY: the training rows and the initial centroids of every level, drawn from one numpy generator.
    -> (S: sorted int64 row indices into X [n_train], init_idx: int32 [M, K] indices into the training rows)."""
    rng = np.random.default_rng(seed)
    n_train = min(int(N), RQ_MAX_POINTS_PER_CENTROID * int(K))
    S = np.sort(rng.permutation(int(N))[:n_train])
    init = np.stack([rng.permutation(n_train)[:K] for _ in range(M)]).astype(np.int32) if n_train >= K else None
    return S, init


def rq_train(ctx: Context, x_train: torch.Tensor, M: int, K: int, init_idx: np.ndarray, niter: int = RQ_NITER):
    """Greedy residual k-means on the device over the training rows ``x_train`` (fp32 [n, d], on ctx's device).
    -> (codebooks: fp32 [M, K, d] on the device, level_mse: float64 [M], the mean |r|^2 of the training rows after each level)."""
    assert x_train.is_cuda and x_train.dtype == torch.float32 and x_train.dim() == 2
    x_train = x_train.contiguous()
    n, d = x_train.shape
    init = np.ascontiguousarray(init_idx, dtype=np.int32)
    if init.shape != (M, K):
        raise ValueError(f"init_idx must be [M, K] = [{M}, {K}], got {init.shape}")
    books = torch.empty((M, K, d), dtype=torch.float32, device=x_train.device)
    mse = (C.c_double * M)()
    check(ctx.lib.rpr_rq_train(ctx.handle, x_train.data_ptr(), n, d, M, K, int(niter),
                               init.ctypes.data_as(C.POINTER(C.c_int32)), books.data_ptr(), mse, _stream_ptr(x_train.device)),
          "rpr_rq_train")
    return books, np.asarray(list(mse), dtype=np.float64)


RQ_MAX_BEAM, RQ_BEAM_PLANE_BYTES = 8, 8 << 30


def rq_encode(ctx: Context, x, codebooks: torch.Tensor, chunk_rows: int = 1 << 20, beam: int = 1):
    """Residual encoding of every row of ``x`` with trained codebooks (fp32 [M, K, d] on the device): the greedy chain
    (``beam`` = 1, ``rpr_rq_encode``), or ``beam`` candidate encodings kept per row through the levels and the best one
    returned (``rpr_rq_encode_beam``, faiss's ``max_beam_size``). A beam lowers ``chunk_rows`` so that the
    two residual planes of a chunk (2 * rows * beam * d * 4 bytes) stay under 8 GB.
    ``x``: a device tensor (encoded chunk by chunk in place), or a host array / np.memmap [N, d] streamed through two pinned
    buffers (the copy of chunk i + 1 runs while chunk i is encoded). -> (codes: uint16 [N, M] host array,
    level_mse: float64 [M], the mean |r|^2 of all rows after each level). The codes do not depend on chunk_rows."""
    assert codebooks.is_cuda and codebooks.dtype == torch.float32 and codebooks.dim() == 3
    books = codebooks.contiguous()
    M, K, d = books.shape
    dev = books.device
    N = int(x.shape[0])
    if x.shape[1] != d:
        raise ValueError(f"rows of width {x.shape[1]} against codebooks of width {d}")
    codes = np.empty((N, M), dtype=np.uint16)
    sse = np.zeros(M, dtype=np.float64)
    part = (C.c_double * M)()
    stream = torch.cuda.current_stream(dev)
    beam = int(beam)
    if beam != 1:
        if not 1 <= beam <= RQ_MAX_BEAM:
            raise ValueError(f"beam must be 1 .. {RQ_MAX_BEAM}, got {beam}")
        chunk_rows = min(int(chunk_rows), RQ_BEAM_PLANE_BYTES // (2 * beam * d * 4))
    chunk_rows = max(1, min(int(chunk_rows), max(N, 1)))
    codes_dev = torch.empty((chunk_rows, M), dtype=torch.int16, device=dev)

    def run(xc: torch.Tensor, lo: int):
        n = xc.shape[0]
        if beam == 1:
            check(ctx.lib.rpr_rq_encode(ctx.handle, xc.data_ptr(), n, d, books.data_ptr(), M, K, codes_dev.data_ptr(), part,
                                        C.c_void_p(stream.cuda_stream)), "rpr_rq_encode")   # synchronises the stream (level sums)
        else:
            check(ctx.lib.rpr_rq_encode_beam(ctx.handle, xc.data_ptr(), n, d, books.data_ptr(), M, K, beam, codes_dev.data_ptr(),
                                             part, C.c_void_p(stream.cuda_stream)), "rpr_rq_encode_beam")   # synchronises too
        sse[:] += np.asarray(list(part))
        with torch.cuda.stream(stream):
            codes[lo:lo + n] = codes_dev[:n].cpu().numpy().view(np.uint16)

    if isinstance(x, torch.Tensor) and x.is_cuda:
        assert x.dtype == torch.float32
        for lo in range(0, N, chunk_rows):
            run(x[lo:lo + chunk_rows].contiguous(), lo)
    else:
        host = [torch.empty((chunk_rows, d), dtype=torch.float32).pin_memory() for _ in range(2)]
        devb = [torch.empty((chunk_rows, d), dtype=torch.float32, device=dev) for _ in range(2)]
        copy_stream = torch.cuda.Stream(dev)
        done = [None, None]
        starts = list(range(0, N, chunk_rows))

        def stage(i: int):
            lo = starts[i]
            n = min(chunk_rows, N - lo)
            b = i & 1
            if done[b] is not None:
                done[b].synchronize()        # the pinned buffer's previous copy has finished
            host[b][:n].numpy()[:] = np.asarray(x[lo:lo + n], dtype=np.float32)
            with torch.cuda.stream(copy_stream):
                devb[b][:n].copy_(host[b][:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            done[b] = ev
            return n

        if starts:
            n_next = stage(0)
        for i, lo in enumerate(starts):   # chunk i is encoded on a helper thread (ctypes drops the GIL) while i + 1 is read
            n = n_next
            b = i & 1
            stream.wait_event(done[b])
            err: List[BaseException] = []

            def work(xc=devb[b][:n], lo=lo):
                try:
                    run(xc, lo)
                except BaseException as e:  # re-raised on the caller's thread
                    err.append(e)

            t = threading.Thread(target=work)
            t.start()
            try:
                if i + 1 < len(starts):
                    n_next = stage(i + 1)
            finally:
                t.join()
            if err:
                raise err[0]
    return codes, sse / max(N, 1)


def embed(model: DeviceModel, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
    """Dense embedding of every text: ``decoder_last_hidden_state[:, 0, :]`` of the encoder plus one decoder position fed
    with the start embedding (reference ``query_encode``, modeling/t5_generative_retriever.py:786-792). -> fp32 [bz, d_model]
    on the model's device. The pass follows the context's precision."""
    dev = model.ctx.device
    ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    bz, Lq = ids.shape
    if Lq % 8 and Lq < 256:   # same bucketing as search(): masked padding columns, identical results
        pad = min(256, (Lq + 7) // 8 * 8) - Lq
        ids = torch.nn.functional.pad(ids, (0, pad)); mask = torch.nn.functional.pad(mask, (0, pad)); Lq += pad
    out = torch.empty((bz, model.d_model), dtype=torch.float32, device=dev)
    check(model.ctx.lib.rpr_embed(model.ctx.handle, model.handle, ids.data_ptr(), mask.data_ptr(), bz, Lq, out.data_ptr(),
                                  _stream_ptr(dev)), "rpr_embed")
    return out


def _codes_on_device(codes, dev) -> torch.Tensor:
    """uint16 codes [N, M] as an int16 device tensor (torch has no device arithmetic on uint16; the bits are what counts)."""
    if isinstance(codes, torch.Tensor):
        if codes.dtype not in (torch.int16, torch.uint16):
            raise ValueError(f"codes must be 16-bit, got {codes.dtype}")
        return codes.view(torch.int16).to(dev).contiguous()
    arr = np.ascontiguousarray(codes)
    if arr.dtype not in (np.uint16, np.int16):
        raise ValueError(f"codes must be 16-bit, got {arr.dtype}")
    return torch.from_numpy(arr.view(np.int16)).to(dev)


def rq_search(ctx: Context, queries, codebooks, codes, topk: int):
    """Top-``topk`` rows of every query by inner product with the decoded codes (``rpr_rq_search``).
    ``queries`` fp32 [Q, d], ``codebooks`` fp32 [M, K, d], ``codes`` uint16 [N, M] (``rq_encode``'s layout): device tensors,
    or host arrays that are uploaded. -> (idx int64 [Q, topk], scores fp32 [Q, topk]) on the device; past N rows the tail
    is idx -1, score -inf."""
    dev = ctx.device
    q = torch.as_tensor(queries, dtype=torch.float32).to(dev).contiguous()
    books = torch.as_tensor(codebooks, dtype=torch.float32).to(dev).contiguous()
    cd = _codes_on_device(codes, dev)
    if q.dim() != 2 or books.dim() != 3 or cd.dim() != 2:
        raise ValueError("queries [Q, d], codebooks [M, K, d] and codes [N, M] expected")
    Q, d = q.shape
    M, K, d2 = books.shape
    if d2 != d or cd.shape[1] != M:
        raise ValueError(f"queries of width {d} and codes of {cd.shape[1]} levels against codebooks {tuple(books.shape)}")
    topk = int(topk)
    idx = torch.empty((Q, max(topk, 0)), dtype=torch.int64, device=dev)
    scores = torch.empty((Q, max(topk, 0)), dtype=torch.float32, device=dev)
    check(ctx.lib.rpr_rq_search(ctx.handle, q.data_ptr(), Q, d, books.data_ptr(), M, K, cd.data_ptr(), cd.shape[0], topk,
                                idx.data_ptr(), scores.data_ptr(), _stream_ptr(dev)), "rpr_rq_search")
    return idx, scores


FLAT_SCRATCH_BYTES = 256 << 20   # csrc/common.h FLAT_SCRATCH_BYTES: the score scratch of one (query chunk, row sub-block)


def flat_search(ctx: Context, queries, x, topk: int, row_base: int = 0, state=None):
    """Exact top-``topk`` rows of every query by inner product with the rows of ``x`` (``rpr_flat_search``).
    ``queries`` fp32 [Q, d] (device tensor or host array), ``x`` fp32 [n, d] device tensor holding the rows ``row_base`` ..
    ``row_base + n - 1`` of the collection. ``state``: the (idx, scores) a previous call returned for other rows of the same
    collection; the result is then the top of the union (the tensors of ``state`` are left as they are).
    -> (idx int64 [Q, topk] of global rows, scores fp32 [Q, topk]) on the device; the tail of a short result is idx -1,
    score -inf. Ties go to the smaller global row, so any partition of the collection chained through ``state`` gives the
    bits of a single call."""
    dev = ctx.device
    q = torch.as_tensor(queries, dtype=torch.float32).to(dev).contiguous()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError("x must be an fp32 device tensor [n, d]")
    x = x.contiguous()
    if q.dim() != 2 or x.dim() != 2:
        raise ValueError("queries [Q, d] and x [n, d] expected")
    Q, d = q.shape
    if x.shape[1] != d:
        raise ValueError(f"queries of width {d} against rows of width {x.shape[1]}")
    topk = int(topk)
    if state is None:
        idx = torch.empty((Q, max(topk, 0)), dtype=torch.int64, device=dev)
        scores = torch.empty((Q, max(topk, 0)), dtype=torch.float32, device=dev)
    else:
        idx = torch.as_tensor(state[0], dtype=torch.int64).to(dev).clone().contiguous()
        scores = torch.as_tensor(state[1], dtype=torch.float32).to(dev).clone().contiguous()
        if idx.shape != (Q, topk) or scores.shape != (Q, topk):
            raise ValueError(f"state of shape {tuple(idx.shape)} / {tuple(scores.shape)} against Q {Q}, topk {topk}")
    check(ctx.lib.rpr_flat_search(ctx.handle, q.data_ptr(), Q, d, x.data_ptr(), x.shape[0], int(row_base), topk, idx.data_ptr(),
                                  scores.data_ptr(), 0 if state is None else 1, _stream_ptr(dev)), "rpr_flat_search")
    return idx, scores


# ---- cross-encoder teacher (rpr_xenc_*) ----------------------------------------------------------------
XENC_MAX_LEN = 512   # attended tokens per sequence the attention kernel takes
# rpr_xenc_set_precision: exact fp32 (default) | f16 matrix operands, fp32 accumulation (the reference's fp16 autocast)
XENC_PRECISIONS = {"f32": 0, "f16": 1}


@dataclass
class XencConfig:
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    d_ff: int
    max_pos: int
    type_vocab: int
    ln_eps: float = 1e-12


# the stacked per-layer tensors of rpr_xenc_desc and the global ones, with their shapes as functions of the config
def xenc_weight_shapes(cfg: XencConfig) -> Dict[str, tuple]:
    H, F, n = cfg.hidden, cfg.d_ff, cfg.layers
    return {
        "word_emb": (cfg.vocab_size, H), "pos_emb": (cfg.max_pos, H), "type_emb": (cfg.type_vocab, H), "emb_ln_w": (H,), "emb_ln_b": (H,),
        "qkv_w": (n, 3 * H, H), "qkv_b": (n, 3 * H), "ao_w": (n, H, H), "ao_b": (n, H), "ln1_w": (n, H), "ln1_b": (n, H),
        "ff1_w": (n, F, H), "ff1_b": (n, F), "ff2_w": (n, H, F), "ff2_b": (n, H), "ln2_w": (n, H), "ln2_b": (n, H),
        "pool_w": (H, H), "pool_b": (H,), "cls_w": (H,), "cls_b": (1,),
    }


class XencModel:
    """The BERT cross-encoder's weights bound to an ``rpr_xenc`` handle. ``weights``: name -> fp32 tensor in the layout of
    ``xenc_weight_shapes`` (q, k, v rows stacked in that order; per-layer tensors stacked over the layers)."""

    def __init__(self, ctx: Context, weights: Dict[str, torch.Tensor], cfg: XencConfig):
        self.ctx, self.cfg = ctx, cfg
        self.handle = None
        self.w: Dict[str, torch.Tensor] = {}
        for name, shape in xenc_weight_shapes(cfg).items():
            if name not in weights:
                raise KeyError(f"cross-encoder weight {name} is missing")
            t = torch.as_tensor(weights[name], dtype=torch.float32)
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"cross-encoder weight {name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
            self.w[name] = t.to(ctx.device).contiguous()
        d = _lib.XencDesc(vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads, d_ff=cfg.d_ff,
                          max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=float(cfg.ln_eps))
        for name, t in self.w.items():
            setattr(d, name, t.data_ptr())
        h = C.c_void_p()
        check(ctx.lib.rpr_xenc_load(ctx.handle, C.byref(d), C.byref(h)), "rpr_xenc_load")
        self.handle = h

    def set_precision(self, precision: str) -> None:
        """``"f32"`` (default) or ``"f16"``: what ``xenc_score`` of this model computes in from now on. The first switch to
        f16 makes f16 copies of the four per-layer weight stacks on the current stream; the library owns them."""
        if precision not in XENC_PRECISIONS:
            raise ValueError(f"cross-encoder precision {precision!r}; one of {sorted(XENC_PRECISIONS)} expected")
        check(self.ctx.lib.rpr_xenc_set_precision(self.ctx.handle, self.handle, XENC_PRECISIONS[precision], _stream_ptr(self.ctx.device)),
              "rpr_xenc_set_precision")

    @property
    def precision(self) -> str:
        code = self.ctx.lib.rpr_xenc_get_precision(self.handle)
        return {v: k for k, v in XENC_PRECISIONS.items()}[code]

    def __del__(self):
        try:
            if self.handle is not None:
                self.ctx.lib.rpr_xenc_free(self.handle)
                self.handle = None
        except Exception:
            pass


def xenc_pack(input_ids, token_type_ids, attention_mask):
    """Padded [bz, L] batch -> the packed form ``rpr_xenc_score`` takes: (ids [T], types [T], positions [T], seq_off
    int32 numpy [bz + 1]). Only attended tokens are kept, in row-major order; a token's position id is its original column,
    so a hole in a mask does not shift the positions after it. The mask is read on the host (a device mask: one ``.cpu()``);
    ids and types are gathered where they live. ``token_type_ids`` None = zeros. A row whose column 0 is masked raises
    ``ValueError``: the pooled token is column 0."""
    mask = torch.as_tensor(attention_mask)
    ids = torch.as_tensor(input_ids)
    if mask.dim() != 2 or ids.shape != mask.shape:
        raise ValueError(f"input_ids {tuple(ids.shape)} and attention_mask {tuple(mask.shape)}: two equal [bz, L] shapes expected")
    keep = mask.cpu() != 0
    if keep.shape[0] and not bool(keep[:, 0].all()):
        bad = (~keep[:, 0]).nonzero().flatten().tolist()
        raise ValueError(f"attention_mask masks column 0 of rows {bad[:8]}: the pooled token of a cross-encoder pair is column 0")
    lens = keep.sum(dim=1)
    seq_off = np.zeros(keep.shape[0] + 1, dtype=np.int32)
    np.cumsum(lens.numpy(), out=seq_off[1:])
    rows, cols = keep.nonzero(as_tuple=True)   # row-major: sequence by sequence, columns ascending
    r, c = rows.to(ids.device), cols.to(ids.device)
    pk_ids = ids[r, c].to(torch.int32)
    if token_type_ids is None:
        pk_types = torch.zeros_like(pk_ids)
    else:
        tt = torch.as_tensor(token_type_ids)
        if tt.shape != ids.shape:
            raise ValueError(f"token_type_ids {tuple(tt.shape)} against input_ids {tuple(ids.shape)}")
        pk_types = tt[rows.to(tt.device), cols.to(tt.device)].to(torch.int32)
    return pk_ids, pk_types, cols.to(torch.int32), seq_off


def xenc_score_packed(model: XencModel, pk_ids, pk_types, pk_pos, seq_off) -> torch.Tensor:
    """``rpr_xenc_score`` on a packed batch (``xenc_pack``) -> fp32 [bz] logits on the model's device. Asynchronous."""
    dev = model.ctx.device
    ids = torch.as_tensor(pk_ids).to(device=dev, dtype=torch.int32).contiguous()
    types = torch.as_tensor(pk_types).to(device=dev, dtype=torch.int32).contiguous()
    pos = torch.as_tensor(pk_pos).to(device=dev, dtype=torch.int32).contiguous()
    off = np.ascontiguousarray(seq_off, dtype=np.int32)
    bz = off.shape[0] - 1
    if bz < 1 or ids.dim() != 1 or ids.shape != types.shape or ids.shape != pos.shape or int(off[-1]) != ids.shape[0]:
        raise ValueError("packed batch: ids, types and positions [T] with T = seq_off[-1], and at least one sequence, expected")
    out = torch.empty((bz,), dtype=torch.float32, device=dev)
    check(model.ctx.lib.rpr_xenc_score(model.ctx.handle, model.handle, ids.data_ptr(), types.data_ptr(), pos.data_ptr(),
                                       off.ctypes.data_as(C.POINTER(C.c_int32)), bz, out.data_ptr(), _stream_ptr(dev)),
          "rpr_xenc_score")
    return out


def xenc_score(model: XencModel, input_ids, token_type_ids, attention_mask) -> torch.Tensor:
    """One logit per (query, passage) row of a padded tokenizer batch -> fp32 [bz] on the model's device. Packs on the way
    (``xenc_pack``), so padding costs nothing. Token, type and position ids outside the model's tables raise ``ValueError``.
    With device tensors the call synchronises twice (the mask's ``.cpu()`` and the range check of ids and types); with the
    host tensors of a tokenizer not at all."""
    cfg = model.cfg
    ids = torch.as_tensor(input_ids)
    if ids.dim() != 2 or ids.shape[0] < 1:
        raise ValueError("input_ids [bz, L] with bz >= 1 expected")
    if ids.shape[1] > cfg.max_pos:
        raise ValueError(f"batch padded to {ids.shape[1]} columns, the model has {cfg.max_pos} positions")
    pk_ids, pk_types, pk_pos, seq_off = xenc_pack(ids, token_type_ids, attention_mask)
    if pk_ids.numel():
        # one small transfer: free for the host tensors a tokenizer hands over (rerank.py), one synchronisation for device tensors
        lo, hi, tlo, thi = torch.stack([pk_ids.min(), pk_ids.max(), pk_types.min().to(pk_ids.device),
                                        pk_types.max().to(pk_ids.device)]).tolist()
        if lo < 0 or hi >= cfg.vocab_size:
            raise ValueError(f"input_ids in [{lo}, {hi}] leave the vocabulary of {cfg.vocab_size}")
        if tlo < 0 or thi >= cfg.type_vocab:
            raise ValueError(f"token_type_ids in [{tlo}, {thi}] leave the {cfg.type_vocab} token types")
    return xenc_score_packed(model, pk_ids, pk_types, pk_pos, seq_off)
