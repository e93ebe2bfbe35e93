"""Thin Python layer over the C ABI (include/hhgt.h): torch tensors provide device memory and the
stream; every computation happens inside libhhgt.so's HIP kernels."""
import collections
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import BLOSC1, BLOSC2, EncodeResultRec, EncodeStats, HhgtError, Layout, check

# default on-disk geometry: one HDF5 chunk = 64 samples x 8192 variants x 2 haplotypes (1 MiB);
# one Blosc2 block = half a sample row of the chunk = 4096 diploid calls (8 KiB -> two 4 KiB byte
# planes: ~10 KiB of LDS per LZ4 workgroup, so ~30 waves stay resident per CU — the kernel is latency /
# issue bound, not HBM bound); typesize 2 = one diploid call
DEFAULT_SC = 64
DEFAULT_VC = 8192
DEFAULT_TYPESIZE = 2
DEFAULT_BLOCKSIZE = 8192


# the selection records of include/hhgt.h as numpy records: derived from the ctypes structures, so there is one description
SEL_DTYPE = np.dtype(_lib.BlockSel)            # hhgt_block_sel
COUNT_SEL_DTYPE = np.dtype(_lib.CountSel)      # hhgt_count_sel
SAMPLE_SEL_DTYPE = np.dtype(_lib.SampleSel)    # hhgt_sample_sel
PLANE_SEL_DTYPE = np.dtype(_lib.PlaneSel)      # hhgt_plane_sel
GATHER_SEL_DTYPE = np.dtype(_lib.GatherSel)    # hhgt_gather_sel

# the element types of a gather_calls table: the kernel copies them as opaque bytes
GATHER_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.float16, torch.bfloat16, torch.int32, torch.float32,
                 torch.int64, torch.float64)


def make_ring_layout(n_samples, ring_cols, sc=DEFAULT_SC, vc=DEFAULT_VC):
    """ring of `ring_cols` chunk columns (streaming: kept indices wrap, see include/hhgt.h)"""
    return Layout(int(n_samples), int(sc), int(vc), int(ring_cols), int(ring_cols) * int(vc))


class PendingEncode:
    """result record of one hhgt_encode_text_async call: pinned host memory the device writes when the call's work
    has run.  .wait() synchronises on the event recorded behind the call and raises what the synchronous call would."""

    def __init__(self):
        self.buf = torch.zeros(C.sizeof(EncodeResultRec), dtype=torch.uint8).pin_memory()
        self.rec = EncodeResultRec.from_address(self.buf.data_ptr())
        self.event = torch.cuda.Event()

    def wait(self):
        self.event.synchronize()
        check(_lib.load().hhgt_encode_result_status(C.c_void_p(self.buf.data_ptr())))
        return self.rec


def make_layout(n_samples, v_capacity, sc=DEFAULT_SC, vc=DEFAULT_VC):
    """chunk-tiled layout; v_capacity is rounded up to a whole number of chunk columns
    (dense: to a multiple of 128)."""
    if vc:
        v_capacity = -(-max(int(v_capacity), 1) // vc) * vc
    else:
        v_capacity = -(-max(int(v_capacity), 1) // 128) * 128
    return Layout(int(n_samples), int(sc), int(vc), 0, int(v_capacity))


def layout_bytes(lay):
    return int(_lib.load().hhgt_layout_bytes(C.byref(lay)))


def planes_bytes(lay):
    """bytes of the bit-plane form of the matrix under `lay` (a quarter of layout_bytes; 0: the layout cannot carry
    planes — variants per chunk must be a multiple of 4096)"""
    return int(_lib.load().hhgt_planes_bytes(C.byref(lay)))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptr_if_any(t):
    """the kernels take NULL for a tensor without elements"""
    return _ptr(t) if t.numel() else None


_Geometry = collections.namedtuple("_Geometry", "Vc Sc n_vc n_sc")


def _geometry(lay):
    """-> (Vc, Sc, n_vc, n_sc): variants and samples per chunk, chunk columns, chunks per column (dense: one chunk)"""
    Vc, Sc = lay.vc or lay.v_capacity, lay.sc or max(lay.n_samples, 1)
    return _Geometry(Vc, Sc, lay.v_capacity // Vc if Vc else 0, -(-lay.n_samples // Sc) if lay.sc else 1)


def _default_blocksize(nbytes, typesize=1):
    """the chunk (or row), at most 8 KiB, in whole elements"""
    blocksize = min(int(nbytes), DEFAULT_BLOCKSIZE)
    return blocksize - blocksize % typesize


def _planes_arg(planes, what="planes: a contiguous int32 tensor [3, n_rows, row_words]"):
    """bit planes as the kernels take them -> (rows, words per row)"""
    if (planes.dtype not in (torch.int32, torch.uint32) or planes.dim() != 3 or planes.shape[0] != 3
            or not planes.is_contiguous()):
        raise ValueError(what)
    return int(planes.shape[1]), int(planes.shape[2])


def _plane_words(planes, w_lo, w_hi):
    """genotype planes and a word range as the plane kernels take them -> (n_rows, words, w_lo, w_hi); w_hi None: all words"""
    n, words = _planes_arg(planes)
    return n, words, int(w_lo), words if w_hi is None else int(w_hi)


def _weights_arg(w, lead, planes):
    """the weights of assoc_sums / score_sums: contiguous float64 [*lead, n_cols] on the planes' device -> n_cols"""
    if (w.dtype != torch.float64 or w.dim() != len(lead) + 1 or tuple(w.shape[:-1]) != lead or not w.is_contiguous()
            or w.device != planes.device):
        raise ValueError(f"w: a contiguous float64 tensor [{', '.join(map(str, lead))}, n_cols] on the planes' device")
    n_cols = int(w.shape[-1])
    if not 0 <= n_cols < 1 << 32:
        raise ValueError(f"n_cols {n_cols}")
    return n_cols


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@dataclass
class EncodeResult:
    G: torch.Tensor            # uint8 view of the chunk-tiled int8 matrix
    layout: Layout
    start: torch.Tensor
    stop: torch.Tensor
    ref: torch.Tensor
    alt: torch.Tensor
    n_kept: int
    stats: dict
    chrom_runs: list = field(default_factory=list)   # [(first_kept_index, name)]
    P: torch.Tensor = None     # bit-plane form of the matrix (include/hhgt.h), when the encode produced that instead of G

    def dense(self):
        """int8 [S, n_kept, 2] torch tensor (device) gathered out of the chunk-tiled buffer."""
        lay = self.layout
        S, n = lay.n_samples, self.n_kept
        if lay.sc == 0 and lay.vc == 0:
            return self.G.view(torch.int8).view(max(S, 1), lay.v_capacity, 2)[:S, :n]
        Vc, Sc, n_vc, n_sc = _geometry(lay)
        g = self.G.view(torch.int8).view(n_vc, n_sc, Sc, Vc, 2).permute(1, 2, 0, 3, 4)
        return g.reshape(n_sc * Sc, n_vc * Vc, 2)[:S, :n]


def bgzf_scan(raw):
    """Member table of a BGZF byte string (host only; `hhgt_bgzf_scan`).  -> dict(data, comp_off, comp_len, isize,
    crc32, consumed): offsets / lengths of the raw DEFLATE payloads, inflated sizes and CRC-32s from the trailers, bytes
    covered by whole members."""
    from ._lib import load
    lib = load()
    data = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw, dtype=np.uint8)
    offs, lens, isz, crcs = [], [], [], []
    pos, cap = 0, 1 << 16
    while pos < data.size:
        co = np.zeros(cap, dtype=np.uint64)
        cl = np.zeros(cap, dtype=np.uint32)
        iz = np.zeros(cap, dtype=np.uint32)
        cr = np.zeros(cap, dtype=np.uint32)
        n, used = C.c_uint64(0), C.c_uint64(0)
        check(lib.hhgt_bgzf_scan(C.c_void_p(data.ctypes.data + pos), data.size - pos, cap, C.c_void_p(co.ctypes.data),
                                 C.c_void_p(cl.ctypes.data), C.c_void_p(iz.ctypes.data), C.c_void_p(cr.ctypes.data),
                                 C.byref(n), C.byref(used)))
        if n.value == 0:
            break
        offs.append(co[:n.value] + np.uint64(pos))
        lens.append(cl[:n.value])
        isz.append(iz[:n.value])
        crcs.append(cr[:n.value])
        pos += used.value
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    return dict(data=data, comp_off=cat(offs, np.uint64), comp_len=cat(lens, np.uint32), isize=cat(isz, np.uint32),
                crc32=cat(crcs, np.uint32), consumed=pos)


class Context:
    """One per (process, GPU).  Wraps hhgt_ctx."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise HhgtError(-6, "no HIP device visible to torch: libhhgt has no CPU path")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        check(self.lib.hhgt_ctx_create(device, C.byref(h)))
        self.h = h
        self.clevel = 5      # hhgt_ctx's default (the reference's compression_opts[4]); set_clevel keeps it in step

    def close(self):
        if getattr(self, "h", None):
            for st in getattr(self, "_streams", []):
                self.lib.hhgt_stream_destroy(self.h, st)
            self._streams = []
            self.lib.hhgt_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- encode --------------------------------------------------------------------------------
    def encode_text(self, text, n_samples, region="", layout=None, v_base=0, out=None):
        """text: uint8 CUDA tensor holding whole VCF lines.  Returns EncodeResult; pass out=
        (a previous EncodeResult) to append at v_base into the same buffers."""
        assert text.is_cuda and text.dtype == torch.uint8 and text.is_contiguous()
        nbytes = text.numel()
        with torch.cuda.device(self.device):
            if out is None:
                if layout is None:
                    # capacity from a line-count bound: a kept line has at least 16 + 2*S bytes
                    bound = nbytes // (16 + 2 * max(n_samples, 0)) + 1
                    layout = make_layout(n_samples, bound)
                G = torch.zeros(max(layout_bytes(layout), 16), dtype=torch.uint8, device=self.device)
                cap = layout.v_capacity
                start = torch.zeros(cap, dtype=torch.int32, device=self.device)
                stop = torch.zeros(cap, dtype=torch.int32, device=self.device)
                ref = torch.zeros(cap, dtype=torch.uint8, device=self.device)
                alt = torch.zeros(cap, dtype=torch.uint8, device=self.device)
                out = EncodeResult(G, layout, start, stop, ref, alt, 0, {})
            st = EncodeStats()
            rc = self.lib.hhgt_encode_text(self.h, _ptr(text), nbytes, (region or "").encode(),
                                           C.byref(out.layout), int(v_base), _ptr(out.G), _ptr(out.start),
                                           _ptr(out.stop), _ptr(out.ref), _ptr(out.alt), C.byref(st), _stream())
            check(rc)
            out.stats = st.asdict()
            out.n_kept = int(v_base) + int(st.n_kept)
            out.chrom_runs = self.chrom_runs()
        return out

    def _encode_async(self, planes, text, n_samples, out, cursor, max_lines, region, pending):
        assert text.is_cuda and text.dtype == torch.uint8 and text.is_contiguous() and (out.P is not None or not planes)
        nbytes = text.numel()
        if max_lines is None:
            max_lines = nbytes // (16 + 2 * max(n_samples, 0)) + 64
        pending = pending or PendingEncode()
        fn, mats = (self.lib.hhgt_encode_text_planes_async, (_ptr(out.P), _ptr(out.G))) if planes else \
            (self.lib.hhgt_encode_text_async, (_ptr(out.G),))
        with torch.cuda.device(self.device):
            check(fn(self.h, _ptr(text), nbytes, (region or "").encode(), C.byref(out.layout), _ptr(cursor), int(max_lines), *mats,
                     _ptr(out.start), _ptr(out.stop), _ptr(out.ref), _ptr(out.alt), C.c_void_p(pending.buf.data_ptr()), _stream()))
            pending.event.record(torch.cuda.current_stream())
        return pending

    def encode_text_async(self, text, n_samples, out, cursor, max_lines=None, region="", pending=None):
        """hhgt_encode_text_async: appends at the device-resident `cursor` (int64 tensor [1]) into `out`'s buffers and
        returns without waiting.  -> PendingEncode (call .wait() once the counts are needed)"""
        return self._encode_async(False, text, n_samples, out, cursor, max_lines, region, pending)

    def pad_tail_cursor(self, res, cursor):
        with torch.cuda.device(self.device):
            check(self.lib.hhgt_pad_tail_cursor(self.h, C.byref(res.layout), _ptr(cursor), _ptr(res.G), _stream()))

    # ---- bit-plane form of the matrix (include/hhgt.h "Bit-plane form": compressor-only consumers) -------------------
    def encode_text_planes_async(self, text, n_samples, out, cursor, max_lines=None, region="", pending=None):
        """hhgt_encode_text_planes_async: like encode_text_async, but the calls land in out.P as two bits per allele;
        out.G (may be None) only receives the bytes of calls beyond 0 / 1 / missing.  -> PendingEncode
        (.rec.reserved = number of such calls)"""
        return self._encode_async(True, text, n_samples, out, cursor, max_lines, region, pending)

    def pad_tail_planes_cursor(self, res, cursor):
        with torch.cuda.device(self.device):
            check(self.lib.hhgt_pad_tail_planes_cursor(self.h, C.byref(res.layout), _ptr(cursor), _ptr(res.P), _stream()))

    def pad_tail_planes(self, res, v_end, vcol_begin=0, vcol_end=None):
        lay = res.layout
        if vcol_end is None:
            vcol_end = -(-max(v_end, 1) // _geometry(lay).Vc)
        with torch.cuda.device(self.device):
            check(self.lib.hhgt_pad_tail_planes(self.h, C.byref(lay), int(v_end), int(vcol_begin), int(vcol_end), _ptr(res.P), _stream()))

    def compress_planes(self, res, col0=0, n_cols=None, fmt=BLOSC2, dst=None, chunk_off=None, sync=True):
        """hhgt_compress_planes: the chunks of column slots [col0, col0 + n_cols) of res (res.P: the planes; res.G or None:
        the int8 matrix whose bytes back the calls beyond 0 / 1 / missing), typesize 2, 8 KiB blocks.
        -> (dst, chunk_off, total_bytes or None) like compress()"""
        lay = res.layout
        Vc, Sc, n_vc, n_sc = _geometry(lay)
        if n_cols is None:
            n_cols = n_vc - col0
        n_chunks = n_cols * n_sc
        chunk_nbytes = Sc * Vc * 2
        with torch.cuda.device(self.device):
            cap = int(self.lib.hhgt_compress_bound(n_chunks, chunk_nbytes, 2, 8192))
            if dst is None:
                dst = torch.empty(cap, dtype=torch.uint8, device=self.device)
            if chunk_off is None:
                chunk_off = torch.zeros(n_chunks + 1, dtype=torch.int64, device=self.device)
            total = C.c_uint64(0)
            check(self.lib.hhgt_compress_planes(self.h, C.byref(lay), _ptr(res.P), _ptr(res.G), int(col0), int(n_cols), fmt, _ptr(dst),
                                                dst.numel(), _ptr(chunk_off), C.byref(total) if sync else None, _stream()))
        return dst, chunk_off, (int(total.value) if sync else None)

    def planes_expand(self, res, col0=0, n_cols=None, out=None):
        """hhgt_planes_expand: planes (+ res.G's bytes for the calls beyond 0 / 1 / missing) of column slots [col0, col0 + n_cols)
        -> the int8 matrix bytes at their place in `out` (a buffer of the int8 layout; default: a new zeroed one)"""
        lay = res.layout
        if n_cols is None:
            n_cols = _geometry(lay).n_vc - col0
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.zeros(layout_bytes(lay), dtype=torch.uint8, device=self.device)
            check(self.lib.hhgt_planes_expand(self.h, C.byref(lay), _ptr(res.P), _ptr(res.G), int(col0), int(n_cols), _ptr(out), _stream()))
        return out

    def chrom_runs(self):
        n = C.c_uint32(0)
        check(self.lib.hhgt_encode_chrom_runs(self.h, 0, None, None, C.byref(n)))
        if n.value == 0:
            return []
        first = np.zeros(n.value, np.uint64)
        names = np.zeros((n.value, 32), np.uint8)
        check(self.lib.hhgt_encode_chrom_runs(self.h, n.value, first.ctypes.data, names.ctypes.data, C.byref(n)))
        return [(int(first[i]), bytes(names[i]).rstrip(b"\0").decode()) for i in range(n.value)]

    def pad_tail(self, res, v_end=None, vcol_begin=0, vcol_end=None):
        lay = res.layout
        v_end = res.n_kept if v_end is None else v_end
        if vcol_end is None:
            vcol_end = -(-max(v_end, 1) // _geometry(lay).Vc)
        with torch.cuda.device(self.device):
            check(self.lib.hhgt_pad_tail(self.h, C.byref(lay), int(v_end), int(vcol_begin), int(vcol_end),
                                         _ptr(res.G), _stream()))

    def create_stream(self, kind):
        """kind "encode" | "compress": the stream pair for running compress of one block beside encode of the next
        (include/hhgt.h hhgt_stream_create: the compress stream is restricted to 3/4 of the CUs) -> torch ExternalStream,
        destroyed with the context"""
        h = C.c_void_p()
        check(self.lib.hhgt_stream_create(self.h, {"encode": 0, "compress": 1, "frame": 2}[kind], C.byref(h)))
        self._streams = getattr(self, "_streams", [])
        self._streams.append(h)
        return torch.cuda.ExternalStream(h.value, device=self.device)

    def set_frame_stream(self, stream):
        """the framing half of every later compress call runs on `stream` (a torch stream; None: back to one stream) while the
        caller's stream goes on with the next call's LZ4 kernels — include/hhgt.h hhgt_set_frame_stream"""
        check(self.lib.hhgt_set_frame_stream(self.h, C.c_void_p(stream.cuda_stream) if stream is not None else None))

    def set_keep_multiallelic(self, on=True):
        """NON-REFERENCE mode: multi-allelic SNP sites pass the record filter (the reference's isSNP drops them);
        genotypes carry allele indices > 1.  Off by default."""
        check(self.lib.hhgt_set_keep_multiallelic(self.h, 1 if on else 0))

    def set_index_mode(self, mode):
        """how the line index finds the newlines of long records: 2 the walk (default), 1 the hop by the bound, 0 the plain
        scan, -1 back to the default (include/hhgt.h hhgt_set_index_mode); results are identical"""
        check(self.lib.hhgt_set_index_mode(self.h, int(mode)))

    def set_clevel(self, clevel):
        """Blosc clevel analogue = candidates tried per position: 1-2: none (offset-1 runs only), 3-4: 1, 5-6: 2 (default 5,
        the reference's setting), 7: 4, 8: 8, 9: 12 and a one-step lazy parse (what pipeline.stream_files / the converter
        write files with)"""
        check(self.lib.hhgt_set_clevel(self.h, int(clevel)))
        self.clevel = int(clevel)

    # ---- codec ---------------------------------------------------------------------------------
    def compress(self, src, chunk_nbytes, typesize=DEFAULT_TYPESIZE, blocksize=None, fmt=BLOSC2,
                 dst=None, chunk_off=None, sync=True):
        """src: uint8 CUDA tensor of n_chunks * chunk_nbytes bytes.
        -> (dst uint8 tensor, chunk_off int64 tensor [n_chunks+1], total_bytes or None)"""
        assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
        chunk_nbytes = int(chunk_nbytes)
        assert src.numel() % chunk_nbytes == 0
        n_chunks = src.numel() // chunk_nbytes
        if blocksize is None:
            blocksize = _default_blocksize(chunk_nbytes, typesize)
        with torch.cuda.device(self.device):
            cap = int(self.lib.hhgt_compress_bound(n_chunks, chunk_nbytes, typesize, blocksize))
            if cap == 0:
                check(-1)
            if dst is None:
                dst = torch.empty(cap, dtype=torch.uint8, device=self.device)
            if chunk_off is None:
                chunk_off = torch.zeros(n_chunks + 1, dtype=torch.int64, device=self.device)
            total = C.c_uint64(0)
            check(self.lib.hhgt_compress_chunks(self.h, _ptr(src), n_chunks, chunk_nbytes, typesize, blocksize,
                                                fmt, _ptr(dst), dst.numel(), _ptr(chunk_off),
                                                C.byref(total) if sync else None, _stream()))
        return dst, chunk_off, (int(total.value) if sync else None)

    def decompress(self, src, chunk_off, n_chunks, chunk_nbytes, typesize=DEFAULT_TYPESIZE, blocksize=None,
                   dst=None):
        """-> (dst uint8 tensor [n_chunks*chunk_nbytes], n_bad)"""
        if blocksize is None:
            blocksize = _default_blocksize(chunk_nbytes, typesize)
        with torch.cuda.device(self.device):
            if dst is None:
                dst = torch.empty(int(n_chunks) * int(chunk_nbytes), dtype=torch.uint8, device=self.device)
            bad = C.c_uint64(0)
            check(self.lib.hhgt_decompress_chunks(self.h, _ptr(src), _ptr(chunk_off), int(n_chunks),
                                                  int(chunk_nbytes), typesize, blocksize, _ptr(dst),
                                                  C.byref(bad), _stream()))
        return dst, int(bad.value)

    def decompress_blocks(self, sel, chunk_nbytes, typesize=DEFAULT_TYPESIZE, blocksize=None, dst=None):
        """gather decode (hhgt_decompress_blocks): sel is a numpy structured array of SEL_DTYPE (device chunk addresses,
        block, decoded byte range [lo, hi), dst_off), uploaded in one copy.  dst: uint8 tensor (default: just large
        enough for the selections).  -> (dst, n_bad)"""
        if blocksize is None:
            blocksize = _default_blocksize(chunk_nbytes, typesize)
        sel = np.ascontiguousarray(sel, dtype=SEL_DTYPE)
        n = len(sel)
        with torch.cuda.device(self.device):
            if dst is None:
                size = int((sel["dst_off"] + sel["hi"] - sel["lo"]).max()) if n else 0
                dst = torch.empty(size, dtype=torch.uint8, device=self.device)
            d_sel = torch.from_numpy(sel.view(np.uint8)).to(self.device) if n else None
            bad = C.c_uint64(0)
            check(self.lib.hhgt_decompress_blocks(self.h, _ptr(d_sel), n, int(chunk_nbytes), typesize, blocksize,
                                                  _ptr(dst), C.byref(bad), _stream()))
        return dst, int(bad.value)

    def _vmask_arg(self, vmask):
        """a variant mask as the row kernels take it -> (device tensor or None, words): None, a uint32 numpy array, or an
        int32 / uint32 device tensor"""
        if vmask is None:
            return None, 0
        if not torch.is_tensor(vmask):
            vmask = torch.from_numpy(np.ascontiguousarray(vmask, dtype=np.uint32).view(np.int32))
        vmask = vmask.to(self.device)
        if vmask.dtype not in (torch.int32, torch.uint32) or vmask.dim() != 1 or not vmask.is_contiguous():
            raise ValueError("vmask: contiguous uint32 words (store.pack_variant_mask)")
        words = vmask.numel()
        if words == 0:      # (a mask without words is still a mask: every selection is past it)
            vmask = torch.zeros(1, dtype=torch.int32, device=self.device)
        return vmask, words

    def _row_kernel(self, fn, sel, sc, vc, typesize, blocksize, out, *args):
        """one call of a row kernel (hhgt_count_alleles, hhgt_count_samples, hhgt_genotype_planes): the selections
        uploaded in one copy, fn(ctx, d_sel, n, sc, vc, typesize, blocksize, *args, &n_bad, stream).  -> (out, n_bad)"""
        n = len(sel)
        with torch.cuda.device(self.device):
            d_sel = torch.from_numpy(sel.view(np.uint8)).to(self.device) if n else None
            bad = C.c_uint64(0)
            check(fn(self.h, _ptr(d_sel), n, int(sc), int(vc), typesize, blocksize, *args, C.byref(bad), _stream()))
        return out, int(bad.value)

    @staticmethod
    def _row_sel(sel, sel_dtype, vc, blocksize):
        """-> (the selections as a contiguous array of sel_dtype, the block size: by default the row's, at most 8 KiB)"""
        if blocksize is None:
            blocksize = _default_blocksize(int(vc) * 2)
        return np.ascontiguousarray(sel, dtype=sel_dtype), blocksize

    def _out_arg(self, tensor, dtype, shape, name, loose=()):
        """an output tensor: the caller's, checked (contiguous; dtype, where uint32 stands for int32; shape, but for the axes in
        `loose`), or zeros"""
        if tensor is None:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        same = tensor.dim() == len(shape) and all(a == b for i, (a, b) in enumerate(zip(tensor.shape, shape)) if i not in loose)
        if tensor.dtype not in ((dtype, torch.uint32) if dtype == torch.int32 else (dtype,)) or not same or not tensor.is_contiguous():
            raise ValueError(f"{name}: a contiguous {str(dtype).split('.')[1]} tensor {list(shape)}")
        return tensor

    def _counts_arg(self, counts, n_out):
        """the counts tensor of count_alleles / count_samples: the caller's, or zeros [n_out(), 4]"""
        if counts is None:
            counts = torch.zeros((int(n_out()), 4), dtype=torch.int32, device=self.device)
        if (counts.dtype not in (torch.int32, torch.uint32) or counts.dim() != 2 or counts.shape[1] != 4
                or not counts.is_contiguous()):
            raise ValueError("counts: a contiguous int32 tensor [n_out, 4]")
        return counts

    def count_alleles(self, sel, sc, vc, n_out=None, typesize=DEFAULT_TYPESIZE, blocksize=None, counts=None):
        """per-variant allele counts (hhgt_count_alleles): sel is a numpy structured array of COUNT_SEL_DTYPE (device
        chunk addresses, block `part` of the rows, row mask, variants [lo, hi), out_row), uploaded in one copy.  The
        counts are ADDED to `counts`, an int32 tensor [n_out, 4] (the kernel's uint32 words; AN, AC, HET, HOM_ALT; default:
        zeros just large enough for the selections), so calls may accumulate into one buffer.  -> (counts, n_bad)"""
        sel, blocksize = self._row_sel(sel, COUNT_SEL_DTYPE, vc, blocksize)
        with torch.cuda.device(self.device):
            counts = self._counts_arg(counts, lambda: n_out if n_out is not None else
                                      int((sel["out_row"] + sel["hi"] - sel["lo"]).max()) if len(sel) else 0)
            return self._row_kernel(self.lib.hhgt_count_alleles, sel, sc, vc, typesize, blocksize, counts,
                                    _ptr(counts), counts.shape[0])

    def count_samples(self, sel, sc, vc, n_out=None, typesize=DEFAULT_TYPESIZE, blocksize=None, vmask=None, counts=None):
        """per-sample counts (hhgt_count_samples): sel is a numpy structured array of SAMPLE_SEL_DTYPE (device chunk
        addresses, block `part` of the rows, row mask, variants [lo, hi), out_row of chunk row 0, mask_word), uploaded in
        one copy.  vmask: None (every variant of the ranges counts) or the variant mask in the block-padded word layout
        (store.pack_variant_mask): a uint32 numpy array, or an int32 / uint32 device tensor.  The counts are ADDED to
        `counts`, an int32 tensor [n_out, 4] (AN, AC, HET, HOM_ALT per sample row; default: zeros just large enough for
        the selections), so calls may accumulate into one buffer.  -> (counts, n_bad)"""
        sel, blocksize = self._row_sel(sel, SAMPLE_SEL_DTYPE, vc, blocksize)
        with torch.cuda.device(self.device):
            counts = self._counts_arg(counts, lambda: n_out if n_out is not None else
                                      int(sel["out_row"].max()) + int(sc) if len(sel) else 0)
            vmask, words = self._vmask_arg(vmask)
            return self._row_kernel(self.lib.hhgt_count_samples, sel, sc, vc, typesize, blocksize, counts,
                                    _ptr(vmask), words, _ptr(counts), counts.shape[0])

    def genotype_planes(self, sel, sc, vc, n_rows=None, row_words=None, typesize=DEFAULT_TYPESIZE, blocksize=None,
                        vmask=None, planes=None):
        """genotype bit planes (hhgt_genotype_planes): sel is a numpy structured array of PLANE_SEL_DTYPE (a sample
        selection plus out_word), uploaded in one copy; vmask as count_samples takes it.  planes: an int32 tensor
        [3, n_rows, row_words] (HET, HOM_REF, HOM_ALT; 32 variants per word) that the caller has zeroed where the
        selections write; default: zeros just large enough for them.  -> (planes, n_bad)"""
        sel, blocksize = self._row_sel(sel, PLANE_SEL_DTYPE, vc, blocksize)
        n = len(sel)
        with torch.cuda.device(self.device):
            if planes is None:
                if n_rows is None:
                    n_rows = int(sel["out_row"].max()) + int(sc) if n else 0
                if row_words is None:
                    row_words = int(sel["out_word"].max()) + -(-(int(blocksize) // 2) // 32) if n else 0
                planes = torch.zeros((3, int(n_rows), int(row_words)), dtype=torch.int32, device=self.device)
            n_rows, row_words = _planes_arg(planes)
            vmask, words = self._vmask_arg(vmask)
            return self._row_kernel(self.lib.hhgt_genotype_planes, sel, sc, vc, typesize, blocksize, planes,
                                    _ptr(vmask), words, _ptr_if_any(planes), n_rows, row_words)

    def gather_calls(self, sel, sc, vc, values=None, out=None, n_rows=None, n_cols=None, row_map=None, vmask=None,
                     typesize=DEFAULT_TYPESIZE, blocksize=None):
        """selected variants as dense columns (hhgt_gather_calls): sel is a numpy structured array of GATHER_SEL_DTYPE (a
        sample selection plus out_col; out_row indexes row_map), uploaded in one copy; vmask as count_samples takes it.
        values: the class table, a contiguous device tensor [4, n_cols] of one of GATHER_DTYPES (rows HOM_REF, HET,
        HOM_ALT, not complete), copied element by element as opaque bytes; None: raw mode, the element is the call's two
        int8 alleles.  row_map: None (chunk row r of a selection goes to output row out_row + r) or the output row of
        every entry, a numpy array or an int32 / uint32 device tensor.  out: [n_rows, row_stride] of the table's dtype, or
        [n_rows, row_stride, 2] int8 in raw mode — dense rows (the last stride 1), a row stride of at least n_cols
        (n_cols: the table's, or by default the width of `out`), any element-aligned address —, of which only the owned
        elements are written; default: zeros just large enough for the selections.  -> (out, n_bad)"""
        sel, blocksize = self._row_sel(sel, GATHER_SEL_DTYPE, vc, blocksize)
        n, raw = len(sel), values is None
        with torch.cuda.device(self.device):
            if not raw:
                if (not torch.is_tensor(values) or values.dtype not in GATHER_DTYPES or values.dim() != 2 or values.shape[0] != 4
                        or not values.is_contiguous() or not values.is_cuda):
                    raise ValueError("values: a contiguous device tensor [4, n_cols] of an 8, 16, 32 or 64 bit type")
                if n_cols is not None and int(n_cols) != values.shape[1]:
                    raise ValueError(f"n_cols {int(n_cols)} with a table of {values.shape[1]} columns")
                n_cols = int(values.shape[1])
            if row_map is not None:
                if not torch.is_tensor(row_map):
                    row_map = torch.from_numpy(np.ascontiguousarray(row_map, dtype=np.uint32).view(np.int32))
                row_map = row_map.to(self.device)
                if row_map.dtype not in (torch.int32, torch.uint32) or row_map.dim() != 1 or not row_map.is_contiguous():
                    raise ValueError("row_map: contiguous uint32 output rows")
            dtype, tail = (torch.int8, (2,)) if raw else (values.dtype, ())
            if out is None:
                if n_rows is None:
                    n_rows = (0 if not n else int(sel["out_row"].max()) + int(sc) if row_map is None else
                              int(row_map.view(torch.int32).max()) + 1 if row_map.numel() else 0)
                if n_cols is None:
                    n_cols = int((sel["out_col"] + sel["hi"] - sel["lo"]).max()) if n else 0
                out = torch.zeros((int(n_rows), int(n_cols)) + tail, dtype=dtype, device=self.device)
            want = f"out: a {str(dtype).split('.')[1]} device tensor [n_rows, row_stride{', 2' if raw else ''}] with dense rows"
            if (not torch.is_tensor(out) or out.dtype != dtype or out.dim() != 2 + len(tail) or tuple(out.shape[2:]) != tail
                    or not out.is_cuda or (n_rows is not None and int(n_rows) != out.shape[0])):
                raise ValueError(want)
            unit = 2 if raw else 1                  # elements of `out` per element of the kernel
            n_cols = int(out.shape[1]) if n_cols is None else int(n_cols)
            stride = out.stride(0) // unit if out.shape[0] > 1 else int(out.shape[1])
            dense = out.stride(-1) == 1 and (not raw or out.stride(1) == 2) and (out.shape[0] <= 1 or out.stride(0) % unit == 0)
            if not dense or n_cols > out.shape[1] or stride < out.shape[1]:
                raise ValueError(want + f" of at least {n_cols} columns")
            vmask, words = self._vmask_arg(vmask)
            return self._row_kernel(self.lib.hhgt_gather_calls, sel, sc, vc, typesize, blocksize, out, _ptr(vmask), words,
                                    _ptr(row_map), 0 if row_map is None else row_map.numel(), _ptr(values),
                                    2 if raw else values.element_size(), _ptr_if_any(out), out.shape[0], n_cols, stride)

    def pair_counts(self, planes, w_lo=0, w_hi=None, table=None):
        """pairwise counts (hhgt_pair_counts) over the words [w_lo, w_hi) (default: all) of genotype planes [3, n, words]:
        ADDED to `table`, an int32 tensor [n, n, 4] (NSNP, HETHET, IBS0, HET1 per ordered pair of rows; default: zeros),
        on the current stream — calls on one stream may accumulate into one table.  -> table"""
        n, words, w_lo, w_hi = _plane_words(planes, w_lo, w_hi)
        with torch.cuda.device(self.device):
            table = self._out_arg(table, torch.int32, (n, n, 4), "table")
            check(self.lib.hhgt_pair_counts(self.h, _ptr_if_any(planes), n, words, w_lo, w_hi, _ptr_if_any(table), _stream()))
        return table

    def grm(self, planes, z, w_lo=0, w_hi=None, table=None):
        """sums of products of standardised dosages (hhgt_grm) over the words [w_lo, w_hi) (default: all) of genotype
        planes [3, n, words]: z is a float32 tensor [3, 32 * words], the value of a HOM_REF, HET, HOM_ALT call at every bit
        position; the sums are ADDED to `table`, a float64 tensor [n, n] (default: zeros), on the current stream — calls
        on one stream may accumulate into one table.  -> table"""
        n, words, w_lo, w_hi = _plane_words(planes, w_lo, w_hi)
        if z.dtype != torch.float32 or tuple(z.shape) != (3, 32 * words) or not z.is_contiguous() or z.device != planes.device:
            raise ValueError(f"z: a contiguous float32 tensor [3, {32 * words}] on the planes' device")
        with torch.cuda.device(self.device):
            table = self._out_arg(table, torch.float64, (n, n), "table")
            check(self.lib.hhgt_grm(self.h, _ptr_if_any(planes), n, words, w_lo, w_hi, _ptr_if_any(z), _ptr_if_any(table),
                                    _stream()))
        return table

    def variant_planes(self, planes, w_lo=0, w_hi=None, vplanes=None):
        """variant-major planes (hhgt_variant_planes) of the words [w_lo, w_hi) (default: all) of genotype planes
        [3, n_rows, words]: an int32 tensor [3, 32 * (w_hi - w_lo), ceil(n_rows / 32)] — HET, COMPLETE, HOM_ALT; row p is
        bit position 32 * w_lo + p of the plane rows, bit r % 32 of word r // 32 is plane row r —, every word of it
        written (default: a new tensor).  -> vplanes"""
        n, words, w_lo, w_hi = _plane_words(planes, w_lo, w_hi)
        with torch.cuda.device(self.device):
            shape = (3, 32 * max(w_hi - w_lo, 0), -(-n // 32))
            if vplanes is None:     # (every word is written: no need for zeros)
                vplanes = torch.empty(shape, dtype=torch.int32, device=self.device)
            vplanes = self._out_arg(vplanes, torch.int32, shape, "vplanes")
            check(self.lib.hhgt_variant_planes(self.h, _ptr_if_any(planes), n, words, w_lo, w_hi, _ptr_if_any(vplanes), _stream()))
        return vplanes

    def ld_counts(self, vplanes, window, table=None):
        """LD counts (hhgt_ld_counts) of the pairs of rows at most `window` apart of variant-major planes [3, n, sw]: ADDED
        to `table`, an int32 tensor [n, window, 8] (store.LD_N ... LD_AA of the pair (row k, row k + 1 + d) at [k, d];
        default: zeros), on the current stream — calls on one stream may accumulate into one table.  -> table"""
        (n, sw), window = _planes_arg(vplanes, "vplanes: a contiguous int32 tensor [3, n_var, sw]"), int(window)
        if not 0 <= window < 1 << 32:
            raise ValueError(f"window {window}")
        with torch.cuda.device(self.device):
            # a window outside 1..1024 is refused by the library (HhgtError, like every other bad argument of a kernel
            # call): the default table is then sized for the nearest valid window and the shape check below stands aside
            if table is None:
                table = torch.zeros((n, max(min(window, 1024), 1), 8), dtype=torch.int32, device=self.device)
            table = self._out_arg(table, torch.int32, (n, window, 8), "table", loose=() if 1 <= window <= 1024 else (1,))
            check(self.lib.hhgt_ld_counts(self.h, _ptr_if_any(vplanes), n, sw, window, _ptr_if_any(table), _stream()))
        return table

    def assoc_sums(self, vplanes, w, sums=None):
        """sums of per-sample weights under the bits (hhgt_assoc_sums) of variant-major planes [3, n, sw]: w is a float64
        tensor [32 * sw, n_cols] (1 <= n_cols <= 64; zeros in the rows of no listed sample); sums, a float64 tensor
        [n, 3, n_cols], gets at [v, k, c] the sum of w[s, c] over the bits s of row v of plane k — every entry written
        (default: a new tensor), on the current stream.  -> sums"""
        n, sw = _planes_arg(vplanes, "vplanes: a contiguous int32 tensor [3, n_var, sw]")
        n_cols = _weights_arg(w, (32 * sw,), vplanes)
        with torch.cuda.device(self.device):
            if sums is None:        # (every entry is written: no need for zeros)
                sums = torch.empty((n, 3, n_cols), dtype=torch.float64, device=self.device)
            sums = self._out_arg(sums, torch.float64, (n, 3, n_cols), "sums")
            check(self.lib.hhgt_assoc_sums(self.h, _ptr_if_any(vplanes), n, sw, _ptr_if_any(w), n_cols, _ptr_if_any(sums),
                                           _stream()))
        return sums

    def quad_forms(self, vplanes, coef, a, q=None):
        """the quadratic form of every variant (hhgt_quad_forms) of variant-major planes [3, n, sw] in one matrix: coef is a
        float64 tensor [n, 3], a float64 [32 * sw, 32 * sw], symmetric (the caller's promise: one triangle is read) and
        finite, zeros in the rows and columns of no listed sample, both contiguous and on the planes' device; q, a float64
        tensor [n], gets x^T a x with x(s) = coef[v, 0] HET + coef[v, 1] COMPLETE + coef[v, 2] HOM_ALT of the bits at s —
        every entry written (default: a new tensor), on the current stream.  -> q"""
        n, sw = _planes_arg(vplanes, "vplanes: a contiguous int32 tensor [3, n_var, sw]")
        for name, t, shape in (("coef", coef, (n, 3)), ("a", a, (32 * sw, 32 * sw))):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != vplanes.device:
                raise ValueError(f"{name}: a contiguous float64 tensor {list(shape)} on the planes' device")
        with torch.cuda.device(self.device):
            if q is None:           # (every entry is written: no need for zeros)
                q = torch.empty((n,), dtype=torch.float64, device=self.device)
            q = self._out_arg(q, torch.float64, (n,), "q")
            check(self.lib.hhgt_quad_forms(self.h, _ptr_if_any(vplanes), n, sw, _ptr_if_any(coef), _ptr_if_any(a), _ptr_if_any(q),
                                           _stream()))
        return q

    def logistic_fit(self, vplanes, valid, X, y, beta0, out=None):
        """per-variant logistic fits (hhgt_logistic_fit) over variant-major planes [3, n, sw]: valid is an int32 tensor [sw]
        with a bit for every position that is a listed sample, X float64 [32 * sw, q] (1 <= q <= 14), y float64 [32 * sw]
        of 0 / 1 and beta0 float64 [q] the null fit, all contiguous and on the planes' device; out, a float64 tensor
        [n, 9], gets the record of every variant (store.REC_*: include/hhgt.h names the fields) — every entry written
        (default: a new tensor), on the current stream.  -> out"""
        n, sw = _planes_arg(vplanes, "vplanes: a contiguous int32 tensor [3, n_var, sw]")
        q = _weights_arg(X, (32 * sw,), vplanes)
        if (valid.dtype not in (torch.int32, torch.uint32) or tuple(valid.shape) != (sw,) or not valid.is_contiguous()
                or valid.device != vplanes.device):
            raise ValueError(f"valid: a contiguous int32 tensor [{sw}] on the planes' device")
        for name, t, shape in (("y", y, (32 * sw,)), ("beta0", beta0, (q,))):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != vplanes.device:
                raise ValueError(f"{name}: a contiguous float64 tensor {list(shape)} on the planes' device")
        with torch.cuda.device(self.device):
            if out is None:         # (every entry is written: no need for zeros)
                out = torch.empty((n, 9), dtype=torch.float64, device=self.device)
            out = self._out_arg(out, torch.float64, (n, 9), "out")
            check(self.lib.hhgt_logistic_fit(self.h, _ptr_if_any(vplanes), n, sw, _ptr_if_any(valid), _ptr_if_any(X), q,
                                             _ptr_if_any(y), _ptr(beta0), _ptr_if_any(out), _stream()))
        return out

    def score_sums(self, planes, w, w_lo=0, w_hi=None, sums=None):
        """sums of per-variant weights under the bits (hhgt_score_sums) of the words [w_lo, w_hi) (default: all) of genotype
        planes [3, n, words]: w is a float64 tensor [3, 32 * words, n_cols] (1 <= n_cols <= 64) — the value of a HOM_REF,
        HET, HOM_ALT call at every bit position, finite inside the words of the range, never read outside them; the sums
        are ADDED to `sums`, a float64 tensor [n, n_cols] (default: zeros), on the current stream — calls on one stream may
        accumulate into one table.  -> sums"""
        n, words, w_lo, w_hi = _plane_words(planes, w_lo, w_hi)
        n_cols = _weights_arg(w, (3, 32 * words), planes)
        with torch.cuda.device(self.device):
            sums = self._out_arg(sums, torch.float64, (n, n_cols), "sums")
            if sums.device != planes.device:
                raise ValueError("sums: on the planes' device")
            check(self.lib.hhgt_score_sums(self.h, _ptr_if_any(planes), n, words, w_lo, w_hi, _ptr_if_any(w), n_cols,
                                           _ptr_if_any(sums), _stream()))
        return sums

    def region_sums(self, planes, w, pieces, runs, n_slots, n_regions, sums=None, wait=True):
        """per-region sums of per-variant weights under the bits (hhgt_region_sums) of genotype planes [3, n, words]: w is a
        float64 tensor [3, 32 * words, n_cols] (1 <= n_cols <= 16), indexed as score_sums' — finite inside the pieces, never
        read outside them; pieces int64 [n_pieces, 4], runs int64 [n_runs, 3] and n_slots are store_plan.plan_regions'
        tables (numpy arrays, which are copied to the device, or contiguous tensors on the planes' device).  The sums of
        the pieces of region g are ADDED to sums[:, g, :] of `sums`, a float64 tensor [n, n_regions, n_cols] (default:
        zeros), on the current stream — calls on one stream may accumulate into one table.  wait: wait for the kernels'
        count of pieces and runs that lie outside the rows, the regions or the slots, and raise if there is one; False
        leaves the call asynchronous, and such a piece is skipped.  -> sums"""
        n, words = _planes_arg(planes)
        n_cols = _weights_arg(w, (3, 32 * words), planes)
        n_slots, n_regions = int(n_slots), int(n_regions)
        if not 0 <= n_slots < 1 << 64 or not 0 <= n_regions < 1 << 64:
            raise ValueError(f"n_slots {n_slots}, n_regions {n_regions}")
        tables = []
        for name, t, fields in (("pieces", pieces, 4), ("runs", runs, 3)):
            if isinstance(t, np.ndarray):
                if t.dtype != np.int64:
                    raise ValueError(f"{name}: an int64 array [n, {fields}]")
                t = torch.from_numpy(np.ascontiguousarray(t)).to(planes.device)
            if (t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != fields or not t.is_contiguous()
                    or t.device != planes.device):
                raise ValueError(f"{name}: a contiguous int64 tensor [n, {fields}] on the planes' device")
            tables.append(t)
        pieces, runs = tables
        with torch.cuda.device(self.device):
            sums = self._out_arg(sums, torch.float64, (n, n_regions, n_cols), "sums")
            if sums.device != planes.device:
                raise ValueError("sums: on the planes' device")
            n_bad = C.c_uint64(0)
            check(self.lib.hhgt_region_sums(self.h, _ptr_if_any(planes), n, words, _ptr_if_any(w), n_cols, _ptr_if_any(pieces),
                                            pieces.shape[0], _ptr_if_any(runs), runs.shape[0], n_slots, n_regions,
                                            _ptr_if_any(sums), C.byref(n_bad) if wait else None, _stream()))
        return sums

    def ld_prune(self, table, r2, keep=None):
        """the greedy walk (hhgt_ld_prune) over one tile: table is an int32 tensor [window + n, window, 8] — hhgt_ld_counts
        over the `window` variants before the tile (rows of zeros where there are none) followed by the tile's n —, keep a
        uint8 tensor [window + n] whose first `window` bytes are the keep flags of those earlier variants (default: zeros:
        a first tile); the call fills keep[window:] with 0 / 1.  -> keep"""
        if (table.dtype not in (torch.int32, torch.uint32) or table.dim() != 3 or table.shape[2] != 8
                or table.shape[0] < table.shape[1] or not table.is_contiguous()):
            raise ValueError("table: a contiguous int32 tensor [window + n, window, 8]")
        window = int(table.shape[1])
        n = int(table.shape[0]) - window
        with torch.cuda.device(self.device):
            keep = self._out_arg(keep, torch.uint8, (window + n,), "keep")
            check(self.lib.hhgt_ld_prune(self.h, _ptr_if_any(table), n, window, float(r2), _ptr_if_any(keep), _stream()))
        return keep

    def ld_decisions(self, table, r2, pos=None, max_dist=None, bits=None):
        """the link bits of one tile (hhgt_ld_decisions), without a walk: table as ld_prune takes it, an int32 tensor
        [window + n, window, 8] whose first `window` rows are carried; pos, an int64 tensor [window + n] laid out like the
        rows, and max_dist >= 0 together set a distance limit (inclusive), neither means none.  bits, an int64 tensor
        [n, ceil(window / 64)] (default: a new one), gets at bit d % 64 of word [k, d // 64] whether the pair (k - 1 - d, k)
        is linked: ld_exceeds of the entry, strictly, and within max_dist — every word written, bits at or past `window`
        0.  -> bits"""
        if (table.dtype not in (torch.int32, torch.uint32) or table.dim() != 3 or table.shape[2] != 8
                or table.shape[0] < table.shape[1] or table.shape[1] < 1 or not table.is_contiguous()):
            raise ValueError("table: a contiguous int32 tensor [window + n, window, 8]")
        window = int(table.shape[1])
        n = int(table.shape[0]) - window
        if (pos is None) != (max_dist is None):
            raise ValueError("pos and max_dist: both or neither")
        if pos is not None and (pos.dtype != torch.int64 or tuple(pos.shape) != (window + n,) or not pos.is_contiguous()
                                or pos.device != table.device):
            raise ValueError(f"pos: a contiguous int64 tensor [{window + n}] on the table's device")
        if max_dist is not None and not 0 <= int(max_dist) < 1 << 63:
            raise ValueError(f"max_dist {max_dist} (at least 0)")
        with torch.cuda.device(self.device):
            shape = (n, -(-window // 64))
            if bits is None:        # (every word is written: no need for zeros)
                bits = torch.empty(shape, dtype=torch.int64, device=self.device)
            bits = self._out_arg(bits, torch.int64, shape, "bits")
            check(self.lib.hhgt_ld_decisions(self.h, _ptr_if_any(table), n, window, float(r2), None if pos is None else _ptr(pos),
                                             0 if max_dist is None else int(max_dist), _ptr_if_any(bits), _stream()))
        return bits

    def ld_clump(self, bits, window, rank, eligible, owner=None):
        """LD clumping from link bits (hhgt_ld_clump): bits an int64 tensor [n, ceil(window / 64)] as ld_decisions writes
        it, for all n counted variants of a group at once; rank an int32 tensor [n] (store_stats.clump_rank: the place in
        a stable ascending sort by p), eligible a uint8 or bool tensor [n] (p <= p1).  owner, an int32 tensor [n]
        (default: a new one), gets per variant its own offset if it is an index variant, the offset of the linked index
        variant of lowest rank if it has one, else -1 — store_stats.clump_reference is the contract.  The call waits for
        the stream.  -> (owner, rounds): rounds the number of rounds that decided at least one variant"""
        window = int(window)
        if not 0 <= window < 1 << 32:
            raise ValueError(f"window {window}")
        nq = -(-max(min(window, 1024), 1) // 64)
        if bits.dtype != torch.int64 or bits.dim() != 2 or bits.shape[1] != nq or not bits.is_contiguous():
            raise ValueError(f"bits: a contiguous int64 tensor [n, {nq}]")
        n = int(bits.shape[0])
        for name, t, dtypes in (("rank", rank, (torch.int32, torch.uint32)), ("eligible", eligible, (torch.uint8, torch.bool))):
            if t.dtype not in dtypes or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != bits.device:
                raise ValueError(f"{name}: a contiguous {str(dtypes[0]).split('.')[1]} tensor [{n}] on the bits' device")
        rounds = C.c_uint32(0)
        with torch.cuda.device(self.device):
            if owner is None:       # (every entry is written: no need for zeros)
                owner = torch.empty((n,), dtype=torch.int32, device=self.device)
            owner = self._out_arg(owner, torch.int32, (n,), "owner")
            check(self.lib.hhgt_ld_clump(self.h, _ptr_if_any(bits), n, window, _ptr_if_any(rank), _ptr_if_any(eligible),
                                         _ptr_if_any(owner), C.byref(rounds), _stream()))
        return owner, int(rounds.value)

    # ---- BGZF on the device -------------------------------------------------------
    def inflate_bgzf(self, raw, return_status=False, check_crc=True):
        """raw: host bytes / uint8 array holding whole BGZF members.  The host walks the member headers
        (bgzf_scan), the compressed bytes are uploaded as they are and every member is inflated by one wave.
        -> (text uint8 tensor on the device, n_bad[, status tensor])"""
        tab = bgzf_scan(raw)
        host = tab["data"]
        n = len(tab["isize"])
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(tab["isize"], dtype=np.uint64, out=out_off[1:])
        total = int(out_off[-1])
        with torch.cuda.device(self.device):
            padded = np.zeros((host.size + 3) // 4 * 4 + 4, dtype=np.uint8)
            padded[:host.size] = host
            d_src = torch.from_numpy(padded).to(self.device)
            d_off = torch.from_numpy(tab["comp_off"]).to(self.device)
            d_len = torch.from_numpy(tab["comp_len"]).to(self.device)
            d_out = torch.from_numpy(out_off[:-1].copy()).to(self.device)
            d_isz = torch.from_numpy(tab["isize"]).to(self.device)
            d_crc = torch.from_numpy(tab["crc32"]).to(self.device) if check_crc else None
            dst = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)[:total]
            status = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)[:n]
            bad = C.c_uint64(0)
            check(self.lib.hhgt_inflate_members(self.h, _ptr(d_src), padded.size, _ptr(d_off), _ptr(d_len), _ptr(d_out),
                                                _ptr(d_isz), n, _ptr(dst), total, _ptr(d_crc), _ptr(status),
                                                C.byref(bad), _stream()))
        return (dst, int(bad.value), status) if return_status else (dst, int(bad.value))

    def inflate_members(self, d_src, src_bytes, d_comp_off, d_comp_len, d_out_off, d_isize, n, dst, dst_bytes, status,
                        count_bad=True, d_crc32=None):
        """`hhgt_inflate_members` on device tensors (see include/hhgt.h) -> number of members flagged in `status`
        (count_bad=False: launch only, no synchronisation, returns None — look at `status` later)"""
        bad = C.c_uint64(0)
        with torch.cuda.device(self.device):
            check(self.lib.hhgt_inflate_members(self.h, _ptr(d_src), int(src_bytes), _ptr(d_comp_off), _ptr(d_comp_len),
                                                _ptr(d_out_off), _ptr(d_isize), int(n), _ptr(dst), int(dst_bytes),
                                                _ptr(d_crc32), _ptr(status), C.byref(bad) if count_bad else None,
                                                _stream()))
        return int(bad.value) if count_bad else None

    # ---- synthetic workloads (bench / test tooling) -----------------------------------------------
    def _synth_text(self, contig, line_lengths, n_samples, with_header, names):
        """what the two renderers begin with: the header, the line offsets behind it, the text buffer with the header in it
        -> (text, off, nbytes)"""
        from . import synth
        head = synth.header_text(contig, names or synth.sample_names(n_samples)) if with_header else b""
        off = np.zeros(len(line_lengths) + 1, dtype=np.uint64)
        off[0] = len(head)
        off[1:] = len(head) + np.cumsum(line_lengths).astype(np.uint64)
        nbytes = int(off[-1])
        text = torch.empty(nbytes + 16, dtype=torch.uint8, device=self.device)
        if head:
            text[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(self.device)
        return text, off, nbytes

    def _up(self, a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(self.device)

    def synth_fixed(self, contig, table, n_samples, seed, v_first=0, with_header=True, names=None):
        """Render a fixed-width synthetic shard directly in HBM.  -> (text uint8 tensor, nbytes)"""
        from . import synth
        S, pos = int(n_samples), table["pos"]
        with torch.cuda.device(self.device):
            text, off, nbytes = self._synth_text(contig, synth.fixed_line_lengths(contig, pos, S), S, with_header, names)
            d_off, d_pos, d_thr = self._up(off, np.int64), self._up(pos, np.int32), self._up(table["thr"], np.int32)
            d_ref, d_alt = torch.from_numpy(table["ref"]).to(self.device), torch.from_numpy(table["alt"]).to(self.device)
            check(self.lib.hhgt_synth_render_fixed(self.h, _ptr(text), nbytes, _ptr(d_off), _ptr(d_pos), _ptr(d_ref), _ptr(d_alt),
                                                   _ptr(d_thr), len(pos), int(v_first), contig.encode(), S, int(seed), _stream()))
            torch.cuda.current_stream().synchronize()
        return text[:nbytes], nbytes

    def synth_mixed(self, contig, table, n_samples, seed, v_first=0, with_header=True, names=None):
        """config-4 style shard (synth.mixed_table) rendered in HBM -> (text uint8 tensor, nbytes, line_off)"""
        from . import synth
        S = int(n_samples)
        with torch.cuda.device(self.device):
            text, off, nbytes = self._synth_text(contig, synth.mixed_line_lengths(contig, table, S), S, with_header, names)
            d_off, d_pos = self._up(off, np.int64), self._up(table["pos"], np.int32)
            d_ref8, d_alt8 = self._up(table["ref8"], np.int64), self._up(table["alt8"], np.int64)
            d_meta, d_thr = self._up(table["meta"], np.int32), self._up(table["thr"], np.int32)
            check(self.lib.hhgt_synth_render_mixed(self.h, _ptr(text), nbytes, _ptr(d_off), _ptr(d_pos), _ptr(d_ref8), _ptr(d_alt8),
                                                   _ptr(d_meta), _ptr(d_thr), len(table["pos"]), int(v_first), contig.encode(), S,
                                                   int(seed), _stream()))
            torch.cuda.current_stream().synchronize()
        return text[:nbytes], nbytes, off

    # ---- profiling -----------------------------------------------------------------------------
    def profile(self, on=True):
        check(self.lib.hhgt_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.hhgt_profile_reset(self.h))

    def profile_read(self):
        ms = (C.c_double * _lib.N_STAGES)()
        n = (C.c_uint64 * _lib.N_STAGES)()
        check(self.lib.hhgt_profile_read(self.h, ms, n))
        return {name: dict(ms=ms[i], launches=int(n[i])) for i, name in enumerate(_lib.STAGE_NAMES) if n[i]}
