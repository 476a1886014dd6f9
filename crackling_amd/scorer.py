"""Host-side mirror of the reference interface for the ISSL scoring step.

`IsslIndex` wraps an index handle of the C ABI; `run_scorer_binary` / `parse_scorer_output` restate
what Crackling's driver does around the scorer process (src/crackling/Crackling.py:747-786): write
`seq[0:20] + "\\n"` per guide, run `<binary> <issl> <query> <maxDist> <threshold> <method> > out`,
split each stdout line on tabs and keep lines with exactly three fields.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from . import _lib
from ._lib import lib, check, IsslError

METHODS = {"unknown": 0, "mit": 1, "cfd": 2, "and": 3, "or": 4, "avg": 5}
# issl_offtarget (40 bytes) and issl_profile (88 bytes) of include/issl_hip.h
OFFTARGET_DTYPE = np.dtype([("site", "<u8"), ("mit", "<f8"), ("cfd", "<f8"), ("guide", "<u4"), ("id", "<u4"), ("occ", "<u4"),
                            ("dist", "<u2"), ("slice", "<u2")])
SEARCH_QUERY_DTYPE = np.dtype([("sig", "<u8"), ("care", "<u8")])  # issl_search_query (16 bytes)
SEARCH_HIT_DTYPE = np.dtype([("site", "<u8"), ("pos", "<u8"), ("record", "<u4"), ("query", "<u4"), ("mism", "<u4"),
                             ("strand", "u1"), ("dist", "u1"), ("reserved", "u1", (2,))])  # issl_search_hit (32 bytes)
VARIANT_HIT_DTYPE = np.dtype([("pos", "<u8"), ("site", "<u4", (4,)), ("record", "<u4"), ("query", "<u4"), ("mism", "<u4"),
                              ("strand", "u1"), ("dist", "u1"), ("n_var", "u1"), ("reserved", "u1")])  # issl_variant_hit (40 bytes)
SNP_DTYPE = np.dtype([("pos", "<u8"), ("record", "<u4"), ("ref", "u1"), ("alt", "u1"), ("reserved", "u1", (2,))])  # issl_snp (16 bytes)
INDEL_DTYPE = np.dtype([("pos", "<u8"), ("record", "<u4"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("ref_at", "<u4"), ("alt_at", "<u4"),
                        ("reserved", "<u4")])  # issl_indel (32 bytes)
HAPLOTYPE_HIT_DTYPE = np.dtype([("pos", "<u8"), ("site", "<u4", (4,)), ("record", "<u4"), ("query", "<u4"), ("mism", "<u4"),
                                ("strand", "u1"), ("dist", "u1"), ("n_var", "u1"), ("reserved", "u1"), ("indel", "<u4"),
                                ("edit_at", "<i4")])  # issl_haplotype_hit (48 bytes)
BULGE_VARIANT_HIT_DTYPE = np.dtype([("pos", "<u8"), ("site", "<u4", (4,)), ("record", "<u4"), ("query", "<u4"), ("mism", "<u4"),
                                    ("strand", "u1"), ("dist", "u1"), ("n_var", "u1"), ("bulge", "i1"), ("at", "u1"),
                                    ("reserved", "u1", (7,))])  # issl_bulge_variant_hit (48 bytes)
BULGE_HIT_DTYPE = np.dtype([("site", "<u8"), ("pos", "<u8"), ("record", "<u4"), ("query", "<u4"), ("mism", "<u4"),
                            ("strand", "u1"), ("dist", "u1"), ("bulge", "i1"), ("at", "u1")])  # issl_bulge_hit (32 bytes)
LOCATION_DTYPE = np.dtype([("pos", "<u8"), ("record", "<u4"), ("strand", "<u4")])  # issl_location (16 bytes)
# issl_occurrence (32 bytes)
OCCURRENCE_DTYPE = np.dtype([("pos", "<u8"), ("record", "<u4"), ("n_perfect", "<u4"), ("aligned", "u1"), ("repeated", "u1"),
                             ("nb", "u1"), ("strand", "u1"), ("owner", "u1"), ("code", "u1"), ("reserved", "u1", (2,)),
                             ("source", "<u4"), ("reserved2", "<u4")])
# issl_guide (32 bytes)
GUIDE_DTYPE = np.dtype([("guide23", "<u8"), ("start", "<u8"), ("record", "<u4"), ("strand", "<u4"), ("seen", "<u4"), ("reserved", "<u4")])
PROFILE_DTYPE = np.dtype([("sites", "<u4", (_lib.PROFILE_BINS,)), ("pad", "<u4"), ("occurrences", "<u8", (_lib.PROFILE_BINS,))])
# issl_landing (64 bytes) and issl_landing_profile (144 bytes); `hits` is transcripts.TRANSCRIPT_HITS_DTYPE
LANDING_DTYPE = np.dtype([("site", "<u8"), ("pos", "<u8"), ("record", "<u4"), ("strand", "<u4"), ("guide", "<u4"), ("rank", "<u4"),
                          ("id", "<u4"), ("occ", "<u4"), ("dist", "<u2"), ("slice", "<u2"), ("pad", "<u4"),
                          ("hits", [("hit", "<u4"), ("total", "<u4"), ("status", "<u4"), ("first", "<u4")])])
LANDING_PROFILE_DTYPE = np.dtype([("located", "<u8", (_lib.PROFILE_BINS,)), ("in_exon", "<u8", (_lib.PROFILE_BINS,)),
                                  ("absent", "<u4", (_lib.PROFILE_BINS,)), ("pad", "<u4")])
assert LANDING_DTYPE.itemsize == 64 and LANDING_PROFILE_DTYPE.itemsize == 144
assert INDEL_DTYPE.itemsize == 32 and HAPLOTYPE_HIT_DTYPE.itemsize == 48


def _method_code(method):
    if isinstance(method, str):
        return lib.issl_method_from_string(method.encode())
    return int(method)


def encode_guides(seqs, seq_len=20):
    """2-bit pack guides (isslScoreOfftargets.cpp:63-71). seqs: iterable of str/bytes of length seq_len."""
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    for s in seqs:
        if len(s) != seq_len:
            raise ValueError(f"guide of length {len(s)}, expected {seq_len}")
    out = np.empty(len(seqs), dtype=np.uint64)
    if seqs:
        check(lib.issl_encode_guides(b"".join(seqs), len(seqs), seq_len, seq_len, out.ctypes.data))
    return out


def decode_guides(sigs, seq_len=20):
    buf = C.create_string_buffer(seq_len + 1)
    out = []
    for s in np.asarray(sigs, dtype=np.uint64):
        check(lib.issl_decode_guide(int(s), seq_len, buf))
        out.append(buf.value.decode())
    return out


def format_scores(sigs, mit, cfd, method, seq_len=20):
    """The scorer's stdout (isslScoreOfftargets.cpp:514-527) for already computed scores."""
    code = _method_code(method)
    want_mit = code in (1, 3, 4, 5)
    want_cfd = code in (2, 3, 4, 5)
    lines = []
    for seq, m, c in zip(decode_guides(sigs, seq_len), mit, cfd):
        lines.append(f"{seq}\t{('%f' % m) if want_mit else '-1'}\t{('%f' % c) if want_cfd else '-1'}\n")
    return "".join(lines)


def format_scores_native(sigs, mit, cfd, method, seq_len=20, threads=0):
    """The same text from the library's own formatter (issl_format_scores: what bin/isslScoreOfftargets prints), as bytes."""
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64)
    mit = np.ascontiguousarray(mit, dtype=np.float64)
    cfd = np.ascontiguousarray(cfd, dtype=np.float64)
    assert len(sigs) == len(mit) == len(cfd)
    from ._lib import Span
    spans, n_spans = C.POINTER(Span)(), C.c_size_t()
    check(lib.issl_format_scores(sigs.ctypes.data, mit.ctypes.data, cfd.ctypes.data, len(sigs), seq_len, _method_code(method),
                                 threads, C.byref(spans), C.byref(n_spans)))
    try:
        return b"".join(C.string_at(spans[i].data, spans[i].len) for i in range(n_spans.value))
    finally:
        lib.issl_free_spans(spans, n_spans)


class IsslIndex:
    """An ISSL index: host arrays (.issl sections) and, after upload(), its HBM image."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self._keep = None  # torch tensor that backs the device image, if any

    # -- construction ------------------------------------------------------------------------
    @classmethod
    def open(cls, path):
        h = C.c_void_p()
        check(lib.issl_index_open(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def from_bytes(cls, data):
        h = C.c_void_p()
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        check(lib.issl_index_from_memory(C.addressof(buf), len(data), C.byref(h)))
        return cls(h)

    @classmethod
    def build_from_text(cls, text, seq_len=20, slice_width=8):
        """isslCreateIndex counterpart; text = sorted sites, one per line."""
        if isinstance(text, str):
            text = text.encode()
        if len(text) % (seq_len + 1):
            raise ValueError("site list is not a multiple of the line length")
        h = C.c_void_p()
        check(lib.issl_index_build_from_text(text, len(text) // (seq_len + 1), seq_len, slice_width, C.byref(h)))
        return cls(h)

    @classmethod
    def build_from_sites(cls, sigs, occ, n_lines=None, seq_len=20, slice_width=8):
        sigs = np.ascontiguousarray(sigs, dtype=np.uint64)
        occ = np.ascontiguousarray(occ, dtype=np.uint32)
        if n_lines is None:
            n_lines = int(occ.sum(dtype=np.uint64))
        h = C.c_void_p()
        check(lib.issl_index_build_from_sites(sigs.ctypes.data, occ.ctypes.data, len(sigs), n_lines, seq_len,
                                              slice_width, C.byref(h)))
        return cls(h)

    @classmethod
    def build_on_device(cls, sigs, occ, device=0, n_lines=None, seq_len=20, slice_width=8, options=None):
        """Like build_from_sites + upload, but the slice lists are built on the GPU (no 48 B/site host arrays).
        options: layout options of the image, e.g. {"compact": 1, "host_cold": 1}."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint64)
        occ = np.ascontiguousarray(occ, dtype=np.uint32)
        if n_lines is None:
            n_lines = int(occ.sum(dtype=np.uint64))
        h = C.c_void_p()
        opts = ",".join(f"{k}={v}" for k, v in (options or {}).items()).encode() or None
        check(lib.issl_index_build_on_device_opt(sigs.ctypes.data, occ.ctypes.data, len(sigs), n_lines, seq_len,
                                                 slice_width, device, opts, C.byref(h)))
        return cls(h)

    @classmethod
    def build_from_device_sites(cls, d_sigs, d_occ, n_lines, device=0, seq_len=20, slice_width=8, options=None):
        """The same for a site table that already sits in the memory of `device`: d_sigs (int64/uint64 view of the packed
        signatures, text order, distinct) and d_occ (int32/uint32 counts) are torch CUDA tensors; nothing of the size of the
        index touches host memory.  The tensors may be freed afterwards."""
        assert d_sigs.is_cuda and d_occ.is_cuda and d_sigs.element_size() == 8 and d_occ.element_size() == 4
        assert d_sigs.is_contiguous() and d_occ.is_contiguous() and d_sigs.numel() == d_occ.numel()
        h = C.c_void_p()
        opts = ",".join(f"{k}={v}" for k, v in (options or {}).items()).encode() or None
        check(lib.issl_index_build_from_device_sites(d_sigs.data_ptr(), d_occ.data_ptr(), d_sigs.numel(), int(n_lines), seq_len,
                                                     slice_width, device, opts, C.byref(h)))
        return cls(h)

    @classmethod
    def build_from_fasta(cls, inputs, slice_width=8, device=0, options=None):
        """Genome FASTA -> uploaded index, the site table built on `device` and never in host memory: the handle of
        build_from_text(extract_offtargets(inputs), 20, slice_width), same bytes, scores and errors.  inputs: a list of
        bytes blobs (FASTA contents) or of paths (str / os.PathLike).  slice_width: 8, 4 or 2.  options: layout options
        of the image, e.g. {"compact": 1}."""
        inputs = list(inputs)
        h = C.c_void_p()
        opts = ",".join(f"{k}={v}" for k, v in (options or {}).items()).encode() or None
        if inputs and all(isinstance(x, (bytes, bytearray, memoryview)) for x in inputs):
            blobs = [bytes(x) for x in inputs]
            files = (C.c_char_p * len(blobs))(*blobs)
            lens = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
            check(lib.issl_index_build_from_fasta(files, lens, len(blobs), slice_width, device, opts, C.byref(h)))
        elif inputs and all(isinstance(x, (str, os.PathLike)) for x in inputs):
            paths = [os.fsencode(x) for x in inputs]
            arr = (C.c_char_p * len(paths))(*paths)
            check(lib.issl_index_build_from_fasta_files(arr, len(paths), slice_width, device, opts, C.byref(h)))
        else:
            raise TypeError("inputs: a non-empty list of bytes blobs or of paths")
        return cls(h)

    @classmethod
    def attach_tensor(cls, tensor):
        """Adopt an HBM image that arrived in a torch uint8 CUDA tensor (e.g. by RCCL broadcast)."""
        h = C.c_void_p()
        check(lib.issl_index_attach_image(tensor.device.index or 0, tensor.data_ptr(), tensor.numel(), C.byref(h)))
        ix = cls(h)
        ix._keep = tensor
        return ix

    # -- properties ---------------------------------------------------------------------------
    @property
    def header(self):
        hd = _lib.Header()
        check(lib.issl_index_header(self._h, C.byref(hd)))
        return {n: int(getattr(hd, n)) for n, _ in hd._fields_}

    def bucket_sizes(self):
        hd = self.header
        n = hd["n_slices"] << hd["slice_width"]
        out = np.empty(n, dtype=np.uint64)
        check(lib.issl_index_bucket_sizes(self._h, out.ctypes.data, n))
        return out

    def write(self, path):
        check(lib.issl_index_write(self._h, os.fsencode(path)))

    def device_bytes(self):
        n = C.c_size_t()
        check(lib.issl_index_device_bytes(self._h, C.byref(n)))
        return n.value

    # -- device -------------------------------------------------------------------------------
    def upload(self, device=0):
        check(lib.issl_index_upload(self._h, device))
        return self

    def upload_into_tensor(self, tensor):
        """Build the HBM image inside a caller-owned torch uint8 CUDA tensor."""
        check(lib.issl_index_upload_into(self._h, tensor.device.index or 0, tensor.data_ptr(), tensor.numel()))
        self._keep = tensor
        return self

    def set_option(self, key, value):
        """Tuning knob of this handle (include/issl_hip.h: issl_index_set_option); no batches may be in flight."""
        check(lib.issl_index_set_option(self._h, str(key).encode(), str(value).encode()))
        return self

    def get_option(self, key):
        v = C.c_longlong()
        check(lib.issl_index_get_option(self._h, str(key).encode(), C.byref(v)))
        return v.value

    def cold(self):
        """(host pointer, bytes) of the pinned host buffer holding the cold sections, (None, 0) when all is in HBM."""
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib.issl_index_cold(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def copy_image_to_tensor(self, tensor):
        """Device-to-device copy of the HBM image into a torch uint8 CUDA tensor (256-byte aligned data pointer)."""
        check(lib.issl_index_copy_image_to(self._h, tensor.data_ptr(), tensor.numel()))
        return tensor

    def has_device_image(self):
        return self.get_option("cold_on_host") >= 0

    def image(self):
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib.issl_index_image(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # -- scoring ------------------------------------------------------------------------------
    def _sigs(self, guides):
        if isinstance(guides, np.ndarray) and guides.dtype == np.uint64:
            return np.ascontiguousarray(guides)
        return encode_guides(guides, self.header["seq_len"])

    def score(self, guides, max_dist=4, threshold=75.0, method="and"):
        """-> (mit, cfd) float64 arrays: 10000/(100+sum) per guide (isslScoreOfftargets.cpp:505-506)."""
        sigs = self._sigs(guides)
        mit = np.empty(len(sigs), dtype=np.float64)
        cfd = np.empty(len(sigs), dtype=np.float64)
        check(lib.issl_score(self._h, sigs.ctypes.data, len(sigs), int(max_dist), float(threshold),
                             _method_code(method), mit.ctypes.data, cfd.ctypes.data))
        return mit, cfd

    def score_device(self, d_guides, d_mit, d_cfd, max_dist=4, threshold=75.0, method="and", stream=None):
        """Guides (int64/uint64 view of packed signatures) and outputs are torch CUDA tensors."""
        check(lib.issl_score_device(self._h, d_guides.data_ptr(), d_guides.numel(), int(max_dist), float(threshold),
                                    _method_code(method), d_mit.data_ptr(), d_cfd.data_ptr(),
                                    C.c_void_p(stream) if stream else None))

    def score_device_async(self, d_guides, d_mit, d_cfd, max_dist=4, threshold=75.0, method="and", stream=None):
        """Enqueue only; call finish() before trusting the outputs."""
        check(lib.issl_score_device_async(self._h, d_guides.data_ptr(), d_guides.numel(), int(max_dist),
                                          float(threshold), _method_code(method), d_mit.data_ptr(), d_cfd.data_ptr(),
                                          C.c_void_p(stream) if stream else None))

    def wait(self, stream):
        """Make `stream` wait for every batch enqueued so far (no host synchronisation)."""
        check(lib.issl_score_wait(self._h, C.c_void_p(stream) if stream else None))

    def finish(self, stream=None):
        """Synchronise the enqueued batches.  Returns False when they must be enqueued again (scratch space grew)."""
        rc = lib.issl_score_finish(self._h, C.c_void_p(stream) if stream else None)
        if rc == -8:
            return False
        check(rc)
        return True

    def dump_hits(self, guides, max_dist=4, threshold=0.0, method="and"):
        """Scored off-targets in the reference's scoring order: array of (guide, slice, pos, id, dist, occ)."""
        sigs = self._sigs(guides)
        n = C.c_size_t()
        check(lib.issl_dump_hits(self._h, sigs.ctypes.data, len(sigs), int(max_dist), float(threshold),
                                 _method_code(method), None, 0, C.byref(n)))
        out = np.empty((n.value, 6), dtype=np.uint32)
        if n.value:
            check(lib.issl_dump_hits(self._h, sigs.ctypes.data, len(sigs), int(max_dist), float(threshold),
                                     _method_code(method), out.ctypes.data, n.value, C.byref(n)))
        return out

    # -- off-target report ---------------------------------------------------------------------
    def offtarget_profile(self, guides, max_dist=4):
        """-> (sites uint32[n, 7], occurrences uint64[n, 7]): per guide and distance, the number of off-target sites and
        the sum of their occurrences (every site within max_dist, no early exit; bins above max_dist are zero)."""
        sigs = self._sigs(guides)
        out = np.zeros(len(sigs), dtype=PROFILE_DTYPE)
        check(lib.issl_offtarget_profile(self._h, sigs.ctypes.data, len(sigs), int(max_dist), out.ctypes.data))
        return np.ascontiguousarray(out["sites"]), np.ascontiguousarray(out["occurrences"])

    def offtargets(self, guides, max_dist=4):
        """-> (offsets uint64[n + 1], records): guide i owns records[offsets[i]:offsets[i + 1]], a structured array
        (OFFTARGET_DTYPE: site, mit, cfd, guide, id, occ, dist, slice) in the reference's scoring order."""
        sigs = self._sigs(guides)
        offsets = np.zeros(len(sigs) + 1, dtype=np.uint64)
        n = C.c_size_t()
        args = (self._h, sigs.ctypes.data, len(sigs), int(max_dist), offsets.ctypes.data)
        check(lib.issl_offtargets(*args, None, 0, C.byref(n)))
        recs = np.empty(n.value, dtype=OFFTARGET_DTYPE)
        if n.value:
            check(lib.issl_offtargets(*args, recs.ctypes.data, n.value, C.byref(n)))
        return offsets, recs

    def offtarget_profile_device(self, d_guides, d_out, max_dist=4, stream=None):
        """d_guides: torch CUDA tensor of packed signatures; d_out: torch CUDA uint8 tensor of 88 bytes per guide
        (PROFILE_DTYPE once copied to the host)."""
        check(lib.issl_offtarget_profile_device(self._h, d_guides.data_ptr(), d_guides.numel(), int(max_dist),
                                                d_out.data_ptr(), C.c_void_p(stream) if stream else None))

    def offtargets_device(self, d_guides, d_offsets, d_recs, max_dist=4, stream=None):
        """d_offsets: int64 CUDA tensor of n + 1 words; d_recs: uint8 CUDA tensor (40 bytes per record, OFFTARGET_DTYPE)
        or None for the counting call.  -> the number of records; nothing is written when they do not fit d_recs."""
        n = C.c_size_t()
        cap = d_recs.numel() * d_recs.element_size() // OFFTARGET_DTYPE.itemsize if d_recs is not None else 0
        check(lib.issl_offtargets_device(self._h, d_guides.data_ptr(), d_guides.numel(), int(max_dist), d_offsets.data_ptr(),
                                         d_recs.data_ptr() if cap else None, cap, C.byref(n),
                                         C.c_void_p(stream) if stream else None))
        return n.value

    # -- off-target landings -------------------------------------------------------------------
    def landings(self, guides, genome, annotation=None, max_dist=4):
        """Where the guides' off-targets lie in `genome` (a Genome on this index's device) and, with `annotation` (an
        Annotation on it), which transcripts each place cuts.  -> (offsets uint64[n + 1], rows): guide i owns
        rows[offsets[i]:offsets[i + 1]], a structured array (LANDING_DTYPE) with the guide's off-targets in record order
        and every off-target's places sorted by (record, pos, strand).  Without an annotation hits is status 1."""
        sigs = self._sigs(guides)
        offsets = np.zeros(len(sigs) + 1, dtype=np.uint64)
        n = C.c_size_t()
        args = (self._h, genome._h, annotation._h if annotation is not None else None, sigs.ctypes.data, len(sigs), int(max_dist),
                offsets.ctypes.data)
        check(lib.issl_offtarget_landings(*args, None, 0, C.byref(n)))
        rows = np.empty(n.value, dtype=LANDING_DTYPE)
        if n.value:
            check(lib.issl_offtarget_landings(*args, rows.ctypes.data, n.value, C.byref(n)))
        return offsets, rows

    def landing_profile(self, guides, genome, annotation=None, max_dist=4):
        """-> LANDING_PROFILE_DTYPE array, one row per guide: per distance the landings of the guide's off-targets, those
        of them inside an exon (0 without an annotation) and the off-target sites that do not occur in `genome`.  No
        landing reaches the host."""
        sigs = self._sigs(guides)
        out = np.zeros(len(sigs), dtype=LANDING_PROFILE_DTYPE)
        check(lib.issl_offtarget_landing_profile(self._h, genome._h, annotation._h if annotation is not None else None,
                                                 sigs.ctypes.data, len(sigs), int(max_dist), out.ctypes.data))
        return out

    def landings_device(self, d_guides, genome, d_offsets, d_rows, annotation=None, max_dist=4, stream=None):
        """d_offsets: int64 CUDA tensor of n + 1 words; d_rows: uint8 CUDA tensor (64 bytes per landing, LANDING_DTYPE) or
        None for the counting call.  -> the number of landings; nothing is written when they do not fit d_rows."""
        n_guides = d_guides.numel()
        if d_offsets.numel() * d_offsets.element_size() < 8 * (n_guides + 1):
            raise ValueError("d_offsets holds fewer than n + 1 64-bit words")
        n = C.c_size_t()
        cap = d_rows.numel() * d_rows.element_size() // LANDING_DTYPE.itemsize if d_rows is not None else 0
        check(lib.issl_offtarget_landings_device(self._h, genome._h, annotation._h if annotation is not None else None,
                                                 d_guides.data_ptr() if n_guides else None, n_guides, int(max_dist),
                                                 d_offsets.data_ptr(), d_rows.data_ptr() if cap else None, cap, C.byref(n),
                                                 C.c_void_p(stream) if stream else None))
        return n.value

    def landing_profile_device(self, d_guides, genome, d_out, annotation=None, max_dist=4, stream=None):
        """d_out: uint8 CUDA tensor of 144 bytes per guide (LANDING_PROFILE_DTYPE once copied to the host)."""
        n_guides = d_guides.numel()
        if d_out.numel() * d_out.element_size() < LANDING_PROFILE_DTYPE.itemsize * n_guides:
            raise ValueError("d_out holds fewer than 144 bytes per guide")
        check(lib.issl_offtarget_landing_profile_device(self._h, genome._h, annotation._h if annotation is not None else None,
                                                        d_guides.data_ptr() if n_guides else None, n_guides, int(max_dist),
                                                        d_out.data_ptr() if n_guides else None,
                                                        C.c_void_p(stream) if stream else None))

    def stats(self):
        st = _lib.Stats()
        check(lib.issl_last_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in st._fields_}

    def count_candidates(self, guides):
        sigs = self._sigs(guides)
        out = C.c_uint64()
        check(lib.issl_count_candidates(self._h, sigs.ctypes.data, len(sigs), C.byref(out)))
        return out.value

    def close(self):
        if self._h:
            lib.issl_index_close(self._h)
            self._h = None
            self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IsslNode:
    """Several GPUs of this node in one process: the index image is uploaded on devices[0], broadcast (RCCL over
    xGMI, peer copies as fallback) and every batch is a queue of chunks, one host thread per device taking the next
    chunk when it has finished its last (scores land in input order)."""

    def __init__(self, index, devices=None):
        self._index = index  # keep the host arrays / root image alive
        h = C.c_void_p()
        if devices is None:
            check(lib.issl_node_create(index._h, None, 0, C.byref(h)))
        else:
            arr = (C.c_int * len(devices))(*devices)
            check(lib.issl_node_create(index._h, arr, len(devices), C.byref(h)))
        self._h = h

    def score(self, guides, max_dist=4, threshold=75.0, method="and"):
        sigs = self._index._sigs(guides)
        mit = np.empty(len(sigs), dtype=np.float64)
        cfd = np.empty(len(sigs), dtype=np.float64)
        check(lib.issl_node_score(self._h, sigs.ctypes.data, len(sigs), int(max_dist), float(threshold),
                                  _method_code(method), mit.ctypes.data, cfd.ctypes.data))
        return mit, cfd

    def shard_times(self):
        """Per device, for the last score(): (milliseconds spent scoring, guides scored)."""
        n = self.info()["n_devices"]
        ms = (C.c_double * n)()
        g = (C.c_uint64 * n)()
        check(lib.issl_node_shard_times(self._h, ms, g, n))
        return list(ms), list(g)

    def info(self):
        inf = _lib.NodeInfo()
        check(lib.issl_node_get_info(self._h, C.byref(inf)))
        return {n: getattr(inf, n) for n, _ in inf._fields_}

    def close(self):
        if self._h:
            lib.issl_node_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def search_prepare(pattern, queries):
    """issl_search_prepare: pattern (str / bytes of 1 to 32 IUPAC codes) and queries (a list of str / bytes of its length
    over ACGTN) -> (the pattern struct, the queries as a SEARCH_QUERY_DTYPE array).  No device needed."""
    pattern = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    texts = [t.encode() if isinstance(t, str) else bytes(t) for t in queries]
    for k, t in enumerate(texts):
        if len(t) != len(pattern):
            raise ValueError(f"query {k} has {len(t)} characters, the pattern has {len(pattern)}")
    pat = _lib.SearchPattern()
    out = np.zeros(len(texts), dtype=SEARCH_QUERY_DTYPE)
    blob = b"".join(texts)
    check(lib.issl_search_prepare(pattern, blob if texts else None, len(texts), len(pattern), C.byref(pat),
                                  out.ctypes.data if texts else None))
    return pat, out


def vcf_snps(vcf, records):
    """issl_vcf_snps: the SNPs of a VCF's text (bytes; plain text, no gzip) for records = [(name, length), ...] as
    Genome.records lists them; CHROM is compared with a name up to its first blank.  -> (a SNP_DTYPE array, one entry per
    usable line in file order, and a dict of counts: lines, snps, alleles_skipped, no_allele, unknown_chrom,
    beyond_record).  No device needed.  A malformed line raises IsslError naming it."""
    vcf = bytes(vcf)
    names = [n.encode() if isinstance(n, str) else bytes(n) for n, _ in records]
    k = len(names)
    c_names = (C.c_char_p * max(k, 1))(*names)
    c_lens = (C.c_size_t * max(k, 1))(*[len(n) for n in names])
    c_lengths = (C.c_uint64 * max(k, 1))(*[int(length) for _, length in records])
    n, counts = C.c_size_t(), _lib.VcfCounts()
    check(lib.issl_vcf_snps(vcf, len(vcf), c_names, c_lens, c_lengths, k, None, 0, C.byref(n), C.byref(counts)))
    out = np.zeros(n.value, dtype=SNP_DTYPE)
    if n.value:
        check(lib.issl_vcf_snps(vcf, len(vcf), c_names, c_lens, c_lengths, k, out.ctypes.data, n.value, C.byref(n), C.byref(counts)))
    return out, {name: int(getattr(counts, name)) for name, _ in counts._fields_}


def vcf_indels(vcf, records):
    """issl_vcf_indels: the indels of a VCF's text (bytes; plain text, no gzip) -- every ALT allele over ACGT that differs
    from REF and is no SNP: deletions, insertions, multi-base substitutions, complex alleles -- for records = [(name,
    length), ...] as Genome.records lists them.  -> (an INDEL_DTYPE array, one entry per allele in file order; the allele
    text as bytes, REF then ALT of every entry, which ref_at / alt_at index; a dict of counts: lines, indels,
    alleles_skipped, no_allele, unknown_chrom, beyond_record, too_long).  No device needed.  A malformed line raises
    IsslError naming it."""
    vcf = bytes(vcf)
    names = [n.encode() if isinstance(n, str) else bytes(n) for n, _ in records]
    k = len(names)
    c_names = (C.c_char_p * max(k, 1))(*names)
    c_lens = (C.c_size_t * max(k, 1))(*[len(n) for n in names])
    c_lengths = (C.c_uint64 * max(k, 1))(*[int(length) for _, length in records])
    n, n_bytes, counts = C.c_size_t(), C.c_size_t(), _lib.VcfIndelCounts()
    args = (vcf, len(vcf), c_names, c_lens, c_lengths, k)
    check(lib.issl_vcf_indels(*args, None, 0, C.byref(n), None, 0, C.byref(n_bytes), C.byref(counts)))
    out = np.zeros(n.value, dtype=INDEL_DTYPE)
    alleles = C.create_string_buffer(max(n_bytes.value, 1))
    if n.value:
        check(lib.issl_vcf_indels(*args, out.ctypes.data, n.value, C.byref(n), alleles, n_bytes.value, C.byref(n_bytes), C.byref(counts)))
    return out, alleles.raw[:n_bytes.value], {name: int(getattr(counts, name)) for name, _ in counts._fields_}


def _search_pattern(pattern):
    return pattern if isinstance(pattern, _lib.SearchPattern) else search_prepare(pattern, [])[0]


def _search_args(pattern, queries):
    if isinstance(queries, np.ndarray) and queries.dtype == SEARCH_QUERY_DTYPE:
        return _search_pattern(pattern), np.ascontiguousarray(queries)
    if isinstance(pattern, _lib.SearchPattern):
        raise TypeError("query texts need the pattern's text")
    return search_prepare(pattern, queries)


def _search_bulges(span, dna_bulge, rna_bulge):
    start, length = span
    return _lib.SearchBulges(int(start), int(length), int(dna_bulge), int(rna_bulge))


class Genome:
    """A genome resident on the GPU that says where sites lie (issl_genome_* of include/issl_hip.h): the records of the
    FASTA inputs as the extraction joins them, 1 B per base of HBM.  A location is a match of the extraction: `pos` is
    its 0-based start inside record `record`; strand 0 is the forward pattern, whose site is seq[pos:pos+20]; strand 1 is
    the reverse pattern, whose site is the reverse complement of seq[pos:pos+20], the first 20 of the 23 matched
    characters."""

    def __init__(self, handle):
        self._h = handle
        n_rec, n_bases = C.c_uint64(), C.c_uint64()
        check(lib.issl_genome_info(self._h, C.byref(n_rec), C.byref(n_bases)))
        self.n_bases = n_bases.value
        self.records = []
        name, name_len, length = C.c_void_p(), C.c_size_t(), C.c_uint64()
        for r in range(n_rec.value):
            check(lib.issl_genome_record(self._h, r, C.byref(name), C.byref(name_len), C.byref(length)))
            self.records.append((C.string_at(name, name_len.value) if name_len.value else b"", length.value))

    @classmethod
    def open(cls, inputs, device=0):
        """inputs: a list of bytes blobs (FASTA contents) or of paths (str / os.PathLike; a lone directory stands for its
        non-hidden entries), as for IsslIndex.build_from_fasta: one input is read by the reference's single-file rules,
        several by its per-file rules."""
        inputs = list(inputs)
        h = C.c_void_p()
        if inputs and all(isinstance(x, (bytes, bytearray, memoryview)) for x in inputs):
            blobs = [bytes(x) for x in inputs]
            files = (C.c_char_p * len(blobs))(*blobs)
            lens = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
            check(lib.issl_genome_open(files, lens, len(blobs), device, C.byref(h)))
        elif inputs and all(isinstance(x, (str, os.PathLike)) for x in inputs):
            paths = [os.fsencode(x) for x in inputs]
            arr = (C.c_char_p * len(paths))(*paths)
            check(lib.issl_genome_open_files(arr, len(paths), device, C.byref(h)))
        else:
            raise TypeError("inputs: a non-empty list of bytes blobs or of paths")
        return cls(h)

    def locate(self, sites):
        """sites: 20-mer strings or a uint64 array of packed signatures (IsslIndex.offtargets()[1]["site"]).
        -> (offsets uint64[n + 1], locs): site k owns locs[offsets[k]:offsets[k + 1]], a structured array
        (LOCATION_DTYPE: pos, record, strand) sorted by (record, pos, strand); a site that does not occur has none."""
        if isinstance(sites, np.ndarray):
            sigs = np.ascontiguousarray(sites, dtype=np.uint64)
        else:
            sigs = encode_guides(sites)
        offsets = np.zeros(len(sigs) + 1, dtype=np.uint64)
        n = C.c_size_t()
        args = (self._h, sigs.ctypes.data, len(sigs), offsets.ctypes.data)
        check(lib.issl_genome_locate(*args, None, 0, C.byref(n)))
        locs = np.empty(n.value, dtype=LOCATION_DTYPE)
        if n.value:
            check(lib.issl_genome_locate(*args, locs.ctypes.data, n.value, C.byref(n)))
        return offsets, locs

    def locate_device(self, d_sites, d_offsets, d_locs, stream=None):
        """d_sites: int64 CUDA tensor of packed signatures; d_offsets: int64 CUDA tensor of n + 1 words; d_locs: uint8 CUDA
        tensor (16 bytes per location, LOCATION_DTYPE) or None for the counting call.  -> the number of locations;
        nothing is written when they do not fit d_locs."""
        n = C.c_size_t()
        cap = d_locs.numel() * d_locs.element_size() // LOCATION_DTYPE.itemsize if d_locs is not None else 0
        check(lib.issl_genome_locate_device(self._h, d_sites.data_ptr(), d_sites.numel(), d_offsets.data_ptr(),
                                            d_locs.data_ptr() if cap else None, cap, C.byref(n),
                                            C.c_void_p(stream) if stream else None))
        return n.value

    # The four call shapes of the search entry points; `extra` is what a unit passes between the pattern and the queries
    # (nothing, or the bulge limits), `after` what it passes behind max_dist (nothing, or max_variants).
    def _search_rows(self, fn, dtype, pattern, extra, queries, max_dist, after=()):
        pat, q = _search_args(pattern, queries)
        offsets = np.zeros(len(q) + 1, dtype=np.uint64)
        n = C.c_size_t()
        args = (self._h, C.byref(pat), *extra, q.ctypes.data if len(q) else None, len(q), int(max_dist), *after,
                offsets.ctypes.data)
        check(fn(*args, None, 0, C.byref(n)))  # the counting call, then the filling call
        hits = np.zeros(n.value, dtype=dtype)
        if n.value:
            check(fn(*args, hits.ctypes.data, n.value, C.byref(n)))
        return offsets, hits

    def _search_counts(self, fn, pattern, extra, queries, max_dist, shape, after=()):
        pat, q = _search_args(pattern, queries)
        counts = np.zeros((len(q),) + shape, dtype=np.uint64)
        check(fn(self._h, C.byref(pat), *extra, q.ctypes.data if len(q) else None, len(q), int(max_dist), *after,
                 counts.ctypes.data if len(q) else None))
        return counts

    def _search_rows_device(self, fn, dtype, pattern, extra, d_queries, max_dist, d_offsets, d_hits, stream, after=()):
        pat = _search_pattern(pattern)
        nq = d_queries.numel() * d_queries.element_size() // SEARCH_QUERY_DTYPE.itemsize
        n = C.c_size_t()
        cap = d_hits.numel() * d_hits.element_size() // dtype.itemsize if d_hits is not None else 0
        check(fn(self._h, C.byref(pat), *extra, d_queries.data_ptr() if nq else None, nq, int(max_dist), *after, d_offsets.data_ptr(),
                 d_hits.data_ptr() if cap else None, cap, C.byref(n), C.c_void_p(stream) if stream else None))
        return n.value

    def _search_counts_device(self, fn, pattern, extra, d_queries, max_dist, d_counts, bins, words, stream, after=()):
        pat = _search_pattern(pattern)
        nq = d_queries.numel() * d_queries.element_size() // SEARCH_QUERY_DTYPE.itemsize
        if d_counts.numel() * d_counts.element_size() < 8 * nq * bins:
            raise ValueError("d_counts holds fewer than " + words + " words")
        check(fn(self._h, C.byref(pat), *extra, d_queries.data_ptr() if nq else None, nq, int(max_dist), *after,
                 d_counts.data_ptr() if nq else None, C.c_void_p(stream) if stream else None))

    def search(self, pattern, queries, max_dist=4):
        """Index-free search (issl_genome_search of include/issl_hip.h).  pattern: 1 to 32 IUPAC codes, or the struct of
        search_prepare(); queries: a list of str / bytes of the pattern's length over ACGTN (N: not compared), or the
        array of search_prepare().  -> (offsets uint64[n + 1], hits): query k owns hits[offsets[k]:offsets[k + 1]], a
        structured array (SEARCH_HIT_DTYPE) sorted by (record, pos, strand).  `pos` is the window's 0-based start on the
        forward strand for both strands; `site` is what the query was compared with (strand 1: the reverse complement of
        the window), `mism` its mismatching positions."""
        return self._search_rows(lib.issl_genome_search, SEARCH_HIT_DTYPE, pattern, (), queries, max_dist)

    def search_profile(self, pattern, queries, max_dist=4):
        """-> uint64 array [n, max_dist + 1]: the hits of query k at distance d, counted on the device."""
        return self._search_counts(lib.issl_genome_search_profile, pattern, (), queries, max_dist, (int(max_dist) + 1,))

    def search_device(self, pattern, d_queries, d_offsets, d_hits, max_dist=4, stream=None):
        """pattern: as for search(); d_queries: CUDA tensor of 16 bytes per query (SEARCH_QUERY_DTYPE, e.g. int64 [n, 2]);
        d_offsets: int64 CUDA tensor of n + 1 words; d_hits: uint8 CUDA tensor (32 bytes per hit, SEARCH_HIT_DTYPE) or None
        for the counting call.  -> the number of hits; nothing is written when they do not fit d_hits."""
        return self._search_rows_device(lib.issl_genome_search_device, SEARCH_HIT_DTYPE, pattern, (), d_queries, max_dist, d_offsets,
                                        d_hits, stream)

    def search_profile_device(self, pattern, d_queries, d_counts, max_dist=4, stream=None):
        """d_counts: int64 CUDA tensor of n * (max_dist + 1) words.  Returns when they are written."""
        self._search_counts_device(lib.issl_genome_search_profile_device, pattern, (), d_queries, max_dist, d_counts, int(max_dist) + 1,
                                   "n * (max_dist + 1)", stream)

    def search_bulges(self, pattern, queries, span, max_dist=4, dna_bulge=1, rna_bulge=1):
        """Search with bulges beside the mismatches (issl_genome_search_bulges of include/issl_hip.h).  pattern and queries:
        as for search(); span: (start, length), the pattern positions where the protospacer lies, never guessed;
        dna_bulge / rna_bulge: the most bases of the site / of the query that pair with nothing, 0..3 each.
        -> (offsets uint64[n + 1], hits): query k owns hits[offsets[k]:offsets[k + 1]], a structured array
        (BULGE_HIT_DTYPE) sorted by (record, pos, strand, bulge).  One row per (query, record, pos, strand, bulge) with the
        least distance over the break points; `bulge` is signed (> 0: DNA, < 0: RNA), `at` the break point inside the span,
        `site` the window of L + bulge bases, `mism` in query coordinates.  Nothing is filtered: a locus that matches
        without a bulge is listed under the other bulges' shifted windows too."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        return self._search_rows(lib.issl_genome_search_bulges, BULGE_HIT_DTYPE, pattern, (C.byref(bg),), queries, max_dist)

    def search_bulges_profile(self, pattern, queries, span, max_dist=4, dna_bulge=1, rna_bulge=1):
        """-> uint64 array [n, rna_bulge + dna_bulge + 1, max_dist + 1]: the rows of query k with bulge b (at index
        b + rna_bulge) at minimum distance d, counted on the device."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        return self._search_counts(lib.issl_genome_search_bulges_profile, pattern, (C.byref(bg),), queries, max_dist,
                                   (int(rna_bulge) + int(dna_bulge) + 1, int(max_dist) + 1))

    def search_bulges_device(self, pattern, d_queries, d_offsets, d_hits, span, max_dist=4, dna_bulge=1, rna_bulge=1, stream=None):
        """search_device() with bulges: d_hits is a uint8 CUDA tensor (32 bytes per row, BULGE_HIT_DTYPE) or None for the
        counting call.  -> the number of rows; nothing is written when they do not fit d_hits."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        return self._search_rows_device(lib.issl_genome_search_bulges_device, BULGE_HIT_DTYPE, pattern, (C.byref(bg),), d_queries, max_dist,
                                        d_offsets, d_hits, stream)

    def search_bulges_profile_device(self, pattern, d_queries, d_counts, span, max_dist=4, dna_bulge=1, rna_bulge=1, stream=None):
        """d_counts: int64 CUDA tensor of n * (rna_bulge + dna_bulge + 1) * (max_dist + 1) words.  Returns when they are
        written."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        self._search_counts_device(lib.issl_genome_search_bulges_profile_device, pattern, (C.byref(bg),), d_queries, max_dist, d_counts,
                                   (int(rna_bulge) + int(dna_bulge) + 1) * (int(max_dist) + 1),
                                   "n * (rna_bulge + dna_bulge + 1) * (max_dist + 1)", stream)

    def search_variants(self, pattern, queries, max_dist=4, max_variants=2):
        """search() on a text with IUPAC ambiguity codes read as sets of bases (issl_genome_search_variants of
        include/issl_hip.h): a window of the 14 codes ACGTRYSWKMBDHV with at most max_variants ambiguous positions hits
        when the least distance over the sequences it stands for is within max_dist.  -> (offsets uint64[n + 1], hits) as
        search(), hits in VARIANT_HIT_DTYPE: `site` is four masks, site[b] bit i set when base b of ACGT is in the set the
        strand reads at i; `n_var` the window's ambiguous positions."""
        return self._search_rows(lib.issl_genome_search_variants, VARIANT_HIT_DTYPE, pattern, (), queries, max_dist, (int(max_variants),))

    def search_variants_profile(self, pattern, queries, max_dist=4, max_variants=2):
        """-> uint64 array [n, max_dist + 1]: the rows of search_variants() of query k at distance d, counted on the device."""
        return self._search_counts(lib.issl_genome_search_variants_profile, pattern, (), queries, max_dist, (int(max_dist) + 1,),
                                   (int(max_variants),))

    def search_variants_device(self, pattern, d_queries, d_offsets, d_hits, max_dist=4, max_variants=2, stream=None):
        """search_device() for search_variants(): d_hits is a uint8 CUDA tensor (40 bytes per row, VARIANT_HIT_DTYPE) or None
        for the counting call.  -> the number of rows; nothing is written when they do not fit d_hits."""
        return self._search_rows_device(lib.issl_genome_search_variants_device, VARIANT_HIT_DTYPE, pattern, (), d_queries, max_dist,
                                        d_offsets, d_hits, stream, (int(max_variants),))

    def search_variants_profile_device(self, pattern, d_queries, d_counts, max_dist=4, max_variants=2, stream=None):
        """d_counts: int64 CUDA tensor of n * (max_dist + 1) words.  Returns when they are written."""
        self._search_counts_device(lib.issl_genome_search_variants_profile_device, pattern, (), d_queries, max_dist, d_counts,
                                   int(max_dist) + 1, "n * (max_dist + 1)", stream, (int(max_variants),))

    def search_bulges_variants(self, pattern, queries, span, max_dist=4, dna_bulge=1, rna_bulge=1, max_variants=2):
        """search_bulges() on a text with IUPAC ambiguity codes read as sets of bases (issl_genome_search_bulges_variants of
        include/issl_hip.h): the window of L + bulge codes ACGTRYSWKMBDHV may hold at most max_variants ambiguous
        positions, its unpaired bases included, and `dist` is the least distance over the sequences it stands for and the
        break points.  -> (offsets uint64[n + 1], hits) as search_bulges(), hits in BULGE_VARIANT_HIT_DTYPE: `site` is four
        masks as in VARIANT_HIT_DTYPE, L + bulge positions; `n_var` the window's ambiguous positions."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        return self._search_rows(lib.issl_genome_search_bulges_variants, BULGE_VARIANT_HIT_DTYPE, pattern, (C.byref(bg),), queries, max_dist,
                                 (int(max_variants),))

    def search_bulges_variants_profile(self, pattern, queries, span, max_dist=4, dna_bulge=1, rna_bulge=1, max_variants=2):
        """-> uint64 array [n, rna_bulge + dna_bulge + 1, max_dist + 1]: the rows of search_bulges_variants() of query k with
        bulge b (at index b + rna_bulge) at minimum distance d, counted on the device."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        return self._search_counts(lib.issl_genome_search_bulges_variants_profile, pattern, (C.byref(bg),), queries, max_dist,
                                   (int(rna_bulge) + int(dna_bulge) + 1, int(max_dist) + 1), (int(max_variants),))

    def search_bulges_variants_device(self, pattern, d_queries, d_offsets, d_hits, span, max_dist=4, dna_bulge=1, rna_bulge=1,
                                      max_variants=2, stream=None):
        """search_bulges_device() for search_bulges_variants(): d_hits is a uint8 CUDA tensor (48 bytes per row,
        BULGE_VARIANT_HIT_DTYPE) or None for the counting call.  -> the number of rows; nothing is written when they do not
        fit d_hits."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        return self._search_rows_device(lib.issl_genome_search_bulges_variants_device, BULGE_VARIANT_HIT_DTYPE, pattern, (C.byref(bg),),
                                        d_queries, max_dist, d_offsets, d_hits, stream, (int(max_variants),))

    def search_bulges_variants_profile_device(self, pattern, d_queries, d_counts, span, max_dist=4, dna_bulge=1, rna_bulge=1,
                                              max_variants=2, stream=None):
        """d_counts: int64 CUDA tensor of n * (rna_bulge + dna_bulge + 1) * (max_dist + 1) words.  Returns when they are
        written."""
        bg = _search_bulges(span, dna_bulge, rna_bulge)
        self._search_counts_device(lib.issl_genome_search_bulges_variants_profile_device, pattern, (C.byref(bg),), d_queries, max_dist,
                                   d_counts, (int(rna_bulge) + int(dna_bulge) + 1) * (int(max_dist) + 1),
                                   "n * (rna_bulge + dna_bulge + 1) * (max_dist + 1)", stream, (int(max_variants),))

    def apply_snps(self, snps):
        """Write SNPs into the resident text as ambiguity codes (issl_genome_apply_snps): snps is a SNP_DTYPE array (record,
        0-based pos, ref as one bit of A C G T = 1 2 4 8, alt as a set of them).  -> the number of places whose byte
        changed.  A ref the text does not hold raises IsslError and leaves the text as it was.  The text stays changed for
        every later call on this handle; locate, occurrences, search and search_bulges skip windows over an ambiguity code."""
        snps = np.ascontiguousarray(snps, dtype=SNP_DTYPE)
        changed = C.c_uint64()
        check(lib.issl_genome_apply_snps(self._h, snps.ctypes.data if len(snps) else None, len(snps), C.byref(changed)))
        return changed.value

    def apply_vcf(self, vcf):
        """apply_snps() for the SNPs of a VCF (bytes, or a path to a plain-text file).  -> the counts of vcf_snps() with
        "changed", the number of places whose byte changed."""
        if not isinstance(vcf, (bytes, bytearray, memoryview)):
            with open(vcf, "rb") as fh:
                vcf = fh.read()
        vcf = bytes(vcf)
        counts, changed = _lib.VcfCounts(), C.c_uint64()
        check(lib.issl_genome_apply_vcf(self._h, vcf, len(vcf), C.byref(counts), C.byref(changed)))
        out = {name: int(getattr(counts, name)) for name, _ in counts._fields_}
        out["changed"] = changed.value
        return out

    def haplotypes(self, indels, alleles, window):
        """The ALT haplotypes of indels as a second resident text (issl_haplotypes_open of include/issl_hip.h): indels is an
        INDEL_DTYPE array (record, 0-based pos, ref_len, alt_len, and where the bases start in `alleles`, bytes over ACGT in
        either case), window the one pattern length (1..32) the handle serves.  Every REF is checked against the resident
        text, where a SNP applied earlier is fine; a REF the text does not hold raises IsslError naming the smallest such
        entry.  -> Haplotypes, a snapshot: SNPs applied to this genome later do not reach it."""
        indels = np.ascontiguousarray(indels, dtype=INDEL_DTYPE)
        alleles = bytes(alleles)
        h = C.c_void_p()
        check(lib.issl_haplotypes_open(self._h, indels.ctypes.data if len(indels) else None, len(indels), alleles if alleles else None,
                                       len(alleles), int(window), C.byref(h)))
        return Haplotypes(h)

    def haplotypes_vcf(self, vcf, window):
        """haplotypes() for the indels of a VCF (bytes, or a path to a plain-text file).  -> (Haplotypes, the counts of
        vcf_indels())."""
        if not isinstance(vcf, (bytes, bytearray, memoryview)):
            with open(vcf, "rb") as fh:
                vcf = fh.read()
        vcf = bytes(vcf)
        h, counts = C.c_void_p(), _lib.VcfIndelCounts()
        check(lib.issl_haplotypes_open_vcf(self._h, vcf, len(vcf), int(window), C.byref(counts), C.byref(h)))
        return Haplotypes(h), {name: int(getattr(counts, name)) for name, _ in counts._fields_}

    def occurrences(self, sites, page_length=0, page_starts=None):
        """The Bowtie step (Crackling.py:600-725) as exact counts.  sites: 20-mer strings or a uint64 array of packed
        signatures, duplicates allowed; page_length: the reference's [bowtie2] page-length (0: one page).  -> structured
        array (OCCURRENCE_DTYPE), one row per site: which of the eight reads site + AGG, CGG, GGG, TGG, AAG, CAG, GAG, TAG
        occur in the genome without a mismatch (`aligned`) and which at least twice (`repeated`), `nb` as the reference
        counts, and the verdict the reference files under this site: `code`, the first occurrence of read 0 (record
        0xFFFFFFFF when there is none) and `source`, the site whose group of SAM lines set it (include/issl_hip.h).
        page_starts: pages of any length in place of page_length, as the pages of a run in batches are -- n_pages + 1
        boundaries from 0 to len(sites), never decreasing; page p is sites[page_starts[p]:page_starts[p + 1]]."""
        if isinstance(sites, np.ndarray):
            sigs = np.ascontiguousarray(sites, dtype=np.uint64)
        else:
            sigs = encode_guides(sites)
        rows = np.zeros(len(sigs), dtype=OCCURRENCE_DTYPE)
        if page_starts is not None:
            starts = np.ascontiguousarray(page_starts, dtype=np.uint64)
            if starts.ndim != 1 or len(starts) == 0:
                raise ValueError("page_starts: n_pages + 1 boundaries")
            check(lib.issl_genome_occurrences_paged(self._h, sigs.ctypes.data if len(sigs) else None, len(sigs), starts.ctypes.data,
                                                    len(starts) - 1, rows.ctypes.data if len(sigs) else None))
            return rows
        check(lib.issl_genome_occurrences(self._h, sigs.ctypes.data if len(sigs) else None, len(sigs), int(page_length),
                                          rows.ctypes.data if len(sigs) else None))
        return rows

    def occurrences_device(self, d_sites, d_rows, page_length=0, stream=None, page_starts=None, page_events=None):
        """d_sites: int64 CUDA tensor of packed signatures (left as it is); d_rows: uint8 CUDA tensor of 32 bytes per site
        (OCCURRENCE_DTYPE); page_starts: None, or a 64-bit integer CUDA tensor of n_pages + 1 boundaries in place of
        page_length; page_events: with page_starts, an int32 CUDA tensor of n_pages words that receives the step's `failed`
        figure of every page (issl_genome_occurrences_paged_events_device).  Returns when the rows are written."""
        n = d_sites.numel()
        if d_rows.numel() * d_rows.element_size() < OCCURRENCE_DTYPE.itemsize * n:
            raise ValueError("d_rows holds fewer than 32 bytes per site")
        stream = C.c_void_p(stream) if stream else None
        if page_starts is not None:
            if page_starts.dim() != 1 or page_starts.numel() == 0 or page_starts.element_size() != 8 or not page_starts.is_contiguous():
                raise ValueError("page_starts: a contiguous tensor of n_pages + 1 64-bit boundaries")
            if page_events is not None:
                if page_events.numel() != page_starts.numel() - 1 or page_events.element_size() != 4 or not page_events.is_contiguous():
                    raise ValueError("page_events: a contiguous tensor of n_pages 32-bit words")
                check(lib.issl_genome_occurrences_paged_events_device(
                    self._h, d_sites.data_ptr() if n else None, n, page_starts.data_ptr(), page_starts.numel() - 1,
                    d_rows.data_ptr() if n else None, page_events.data_ptr() if page_events.numel() else None, stream))
                return
            check(lib.issl_genome_occurrences_paged_device(self._h, d_sites.data_ptr() if n else None, n, page_starts.data_ptr(),
                                                           page_starts.numel() - 1, d_rows.data_ptr() if n else None, stream))
            return
        if page_events is not None:
            raise ValueError("page_events needs page_starts")
        check(lib.issl_genome_occurrences_device(self._h, d_sites.data_ptr() if n else None, n, int(page_length),
                                                 d_rows.data_ptr() if n else None, stream))

    def close(self):
        if self._h:
            lib.issl_genome_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Haplotypes:
    """The ALT haplotypes of a set of indels, resident on the GPU as strips of text (issl_haplotypes_* of
    include/issl_hip.h; Genome.haplotypes makes it).  The searches are Genome.search_variants* on the ALT haplotype of one
    indel at a time, at the windows that overlap its edit; rows are in HAPLOTYPE_HIT_DTYPE: the variant search's fields,
    `indel` the input index, `record` and `pos` in reference coordinates, `edit_at` the window index of the first ALT base
    (or of the first base behind a deletion's junction; negative when the window starts inside the ALT allele).  Nothing
    is filtered, two indels are never combined, and there are no bulges: the strips serve one window length."""

    _search_rows = Genome._search_rows
    _search_counts = Genome._search_counts
    _search_rows_device = Genome._search_rows_device
    _search_counts_device = Genome._search_counts_device

    def __init__(self, handle):
        self._h = handle

    def info(self):
        """-> {"n_indels", "text_bytes" (of the strip text, separators included), "window"}."""
        n, text, window = C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(lib.issl_haplotypes_info(self._h, C.byref(n), C.byref(text), C.byref(window)))
        return {"n_indels": n.value, "text_bytes": text.value, "window": window.value}

    def search(self, pattern, queries, max_dist=4, max_variants=2):
        """-> (offsets uint64[n + 1], hits in HAPLOTYPE_HIT_DTYPE): query k owns hits[offsets[k]:offsets[k + 1]], sorted by
        (indel, offset of the window in its strip, strand).  The pattern's length must be the handle's window."""
        return self._search_rows(lib.issl_haplotypes_search, HAPLOTYPE_HIT_DTYPE, pattern, (), queries, max_dist, (int(max_variants),))

    def search_profile(self, pattern, queries, max_dist=4, max_variants=2):
        """-> uint64 array [n, max_dist + 1]: the rows of search() of query k at distance d, counted on the device."""
        return self._search_counts(lib.issl_haplotypes_search_profile, pattern, (), queries, max_dist, (int(max_dist) + 1,),
                                   (int(max_variants),))

    def search_device(self, pattern, d_queries, d_offsets, d_hits, max_dist=4, max_variants=2, stream=None):
        """Genome.search_device() for search(): d_hits is a uint8 CUDA tensor (48 bytes per row, HAPLOTYPE_HIT_DTYPE) or None
        for the counting call.  -> the number of rows; nothing is written when they do not fit d_hits."""
        return self._search_rows_device(lib.issl_haplotypes_search_device, HAPLOTYPE_HIT_DTYPE, pattern, (), d_queries, max_dist,
                                        d_offsets, d_hits, stream, (int(max_variants),))

    def search_profile_device(self, pattern, d_queries, d_counts, max_dist=4, max_variants=2, stream=None):
        """d_counts: int64 CUDA tensor of n * (max_dist + 1) words.  Returns when they are written."""
        self._search_counts_device(lib.issl_haplotypes_search_profile_device, pattern, (), d_queries, max_dist, d_counts,
                                   int(max_dist) + 1, "n * (max_dist + 1)", stream, (int(max_variants),))

    def close(self):
        if self._h:
            lib.issl_haplotypes_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceArray:
    """Device memory of a handle as torch sees it (the CUDA array interface): torch.as_tensor() wraps it without a copy
    and keeps this object, and with it the owner, alive."""

    def __init__(self, owner, ptr, shape, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}


class GuideSet:
    """The candidate guides of FASTA inputs, extracted on the GPU and resident there (issl_guides_* of include/issl_hip.h):
    Crackling's extraction step (Crackling.py:151-305).  Distinct 23-mers in the order the reference first meets them;
    `record`, `start` and `strand` are the place of the first occurrence (strand 1: the guide is the reverse complement
    of seq[start:start+23]), `seen` the number of occurrences; seen == 1 is the reference's isUnique."""

    def __init__(self, handle, device=0):
        self._h = handle
        self.device = device
        n_guides, n_unique, n_matches, n_rec = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.issl_guides_info(self._h, C.byref(n_guides), C.byref(n_unique), C.byref(n_matches), C.byref(n_rec)))
        self.n_guides, self.n_unique, self.n_matches = n_guides.value, n_unique.value, n_matches.value
        self.records = []
        name, name_len, length = C.c_void_p(), C.c_size_t(), C.c_uint64()
        for r in range(n_rec.value):
            check(lib.issl_guides_record(self._h, r, C.byref(name), C.byref(name_len), C.byref(length)))
            self.records.append((C.string_at(name, name_len.value) if name_len.value else b"", length.value))
        self._guides = self._file_counts = None

    @classmethod
    def extract(cls, inputs, device=0):
        """inputs: a list of bytes blobs (FASTA contents) or of paths (str / os.PathLike), read in the order given; a lone
        directory stands for the files in it in reverse sorted name order, as the reference reads it."""
        inputs = list(inputs)
        h = C.c_void_p()
        if inputs and all(isinstance(x, (bytes, bytearray, memoryview)) for x in inputs):
            blobs = [bytes(x) for x in inputs]
            files = (C.c_char_p * len(blobs))(*blobs)
            lens = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
            check(lib.issl_guides_extract(files, lens, len(blobs), device, C.byref(h)))
        elif inputs and all(isinstance(x, (str, os.PathLike)) for x in inputs):
            paths = [os.fsencode(x) for x in inputs]
            arr = (C.c_char_p * len(paths))(*paths)
            check(lib.issl_guides_extract_files(arr, len(paths), device, C.byref(h)))
        else:
            raise TypeError("inputs: a non-empty list of bytes blobs or of paths")
        return cls(h, device)

    def __len__(self):
        return self.n_guides

    @property
    def guides(self):
        """Structured array (GUIDE_DTYPE) of the guides in first-seen order; copied from the device once."""
        if self._guides is None:
            out = np.empty(self.n_guides, dtype=GUIDE_DTYPE)
            check(lib.issl_guides_copy(self._h, out.ctypes.data, len(out)))
            self._guides = out
        return self._guides

    @property
    def file_counts(self):
        """uint32 array [n_inputs, 4], counted during the extraction (issl_guides_file_counts): per input, in the order the
        inputs were read, its matches, those of them that met a guide seen before, the guides whose second occurrence lies
        in it and the guides whose first occurrence lies in it.  What the reference's log prints per file
        (Crackling.py:254-258): its two running figures are the sums of the last two columns over the inputs so far."""
        if self._file_counts is None:
            n, out, rows = C.c_uint64(), (C.c_uint32 * 4)(), []
            check(lib.issl_guides_files(self._h, C.byref(n)))
            for f in range(n.value):
                check(lib.issl_guides_file_counts(self._h, f, out))
                rows.append(list(out))
            self._file_counts = np.array(rows, dtype=np.uint32).reshape(-1, 4)
        return self._file_counts

    def strings(self):
        """The 23-mers as str, in first-seen order."""
        return decode_guides(self.guides["guide23"], 23)

    def _pointers(self):
        d_guides, d_sigs = C.c_void_p(), C.c_void_p()
        check(lib.issl_guides_device(self._h, C.byref(d_guides), C.byref(d_sigs)))
        return d_guides.value, d_sigs.value

    def sigs_tensor(self):
        """int64 CUDA tensor over the set's own signature array (packed guide[0:20] per guide): no copy; the tensor keeps
        the set alive, and close() must not be called while it is in use."""
        import torch
        if not self.n_guides:
            return torch.empty(0, dtype=torch.int64, device=f"cuda:{self.device}")
        return torch.as_tensor(_DeviceArray(self, self._pointers()[1], (self.n_guides,), "<i8"), device=f"cuda:{self.device}")

    def guides_tensor(self):
        """int32 CUDA tensor [n_guides, 8] over the set's own guide records (GUIDE_DTYPE as 32-bit words: column 6 is
        `seen`): no copy."""
        import torch
        if not self.n_guides:
            return torch.empty((0, 8), dtype=torch.int32, device=f"cuda:{self.device}")
        return torch.as_tensor(_DeviceArray(self, self._pointers()[0], (self.n_guides, 8), "<i4"), device=f"cuda:{self.device}")

    def consensus(self, config=None, **kw):
        """The efficiency consensus over this set (Crackling.py:306-598, crackling_amd.Consensus): config is a mapping of
        Consensus's keywords (optimisation, n, mm10db, chopchop, sgrnascorer2, model, sgrna_threshold, low_energy,
        high_energy); keywords given directly win."""
        from .consensus import Consensus
        return Consensus(self, **{**dict(config or {}), **kw})

    def score(self, index, max_dist=4, threshold=75.0, method="and", only_unique=True, consensus=None,
              bowtie=None):
        """Score the guides against an uploaded IsslIndex without taking them through the host: the rows to score are
        selected on the device (only_unique: those with seen == 1, the ones the reference scores at optimisation `low`;
        consensus: a finished Consensus of this set -- its selection, the rows the reference scores at the configured
        optimisation level, and only_unique is not looked at; bowtie: a BowtieStep of that consensus -- the selection
        without the rows Bowtie rejected, as the reference's filter leaves them at medium and high) and their signatures
        go to index.score_device.  The selection makes the host wait for the device once (torch.nonzero has to learn how
        many rows there are); no guide is copied.  -> (idx, mit, cfd) as numpy arrays: idx = the rows of .guides that
        were scored, ascending."""
        import torch
        sigs = self.sigs_tensor()
        if consensus is not None:
            if consensus.guide_set is not self:
                raise ValueError("the consensus belongs to another guide set")
            if bowtie is not None and bowtie.consensus is not consensus:
                raise ValueError("the Bowtie step belongs to another consensus")
            idx = (bowtie if bowtie is not None else consensus).selected_tensor().to(torch.int64)
            sigs = sigs[idx]
        elif bowtie is not None:
            raise ValueError("bowtie: only together with its consensus")
        elif only_unique:
            idx = torch.nonzero(self.guides_tensor()[:, 6] == 1).flatten()
            sigs = sigs[idx]
        else:
            idx = torch.arange(self.n_guides, dtype=torch.int64, device=sigs.device)
        mit = torch.empty(sigs.numel(), dtype=torch.float64, device=sigs.device)
        cfd = torch.empty_like(mit)
        if sigs.numel():
            index.score_device(sigs.contiguous(), mit, cfd, max_dist, threshold, method,
                               stream=torch.cuda.current_stream(sigs.device).cuda_stream)
        return idx.cpu().numpy(), mit.cpu().numpy(), cfd.cpu().numpy()

    def close(self):
        if self._h:
            lib.issl_guides_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def extract_offtargets(fasta_blobs, device=0):
    """Sorted site list (bytes, one 20-mer per line) of FASTA / multi-FASTA contents -- the GPU counterpart of
    crackling/utils/extractOfftargets.py.  fasta_blobs: iterable of bytes; one blob is read by the reference's
    single-file rules, several by its per-file rules ("Index preparation")."""
    blobs = [b if isinstance(b, bytes) else b.encode() for b in fasta_blobs]
    files = (C.c_char_p * len(blobs))(*blobs)
    lens = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    out = C.c_void_p()
    n = C.c_size_t()
    sites = C.c_uint64()
    check(lib.issl_extract_from_memory(files, lens, len(blobs), device, C.byref(out), C.byref(n), C.byref(sites)))
    data = C.string_at(out, n.value) if n.value else b""
    lib.issl_free(out)
    return data


def run_scorer_binary(binary, issl_path, guides23, max_dist, threshold, method, workdir=None, env=None):
    """What Crackling.py:747-778 does for one page of guides: returns the scorer's stdout text.

    guides23: iterable of target strings; only the first 20 characters are written (:751)."""
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        inp = os.path.join(tmp, "offtargetscore.input")
        outp = os.path.join(tmp, "offtargetscore.output")
        with open(inp, "w") as fh:
            for g in guides23:
                fh.write(g[0:20] + "\n")
        cmd = f"{binary} {issl_path} {inp} {max_dist} {threshold} {method} > {outp}"
        subprocess.run(cmd, shell=True, check=True, env=env)  # Helpers.py:39-42
        with open(outp) as fh:
            return fh.read()


def parse_scorer_output(text):
    """Crackling.py:780-786: {sequence: {"mit": float, "cfd": float}} from 3-field lines."""
    out = {}
    for line in text.splitlines():
        parts = line.strip().split("\t")
        if len(parts) == 3:
            out[parts[0]] = {"mit": float(parts[1]), "cfd": float(parts[2])}
    return out


def verdicts(mit, cfd, threshold, method):
    """Crackling.py:780-835 on arrays: 1 = accepted, 0 = rejected, 255 = no rule matches the method name.

    `method` is the configured string (the scorer matches it exactly, the caller lower-cases it)."""
    mit = np.ascontiguousarray(mit, dtype=np.float64)
    cfd = np.ascontiguousarray(cfd, dtype=np.float64)
    if mit.shape != cfd.shape or mit.ndim != 1:
        raise ValueError("mit and cfd must be 1-D arrays of the same length")
    out = np.empty(len(mit), dtype=np.uint8)
    check(lib.issl_verdicts(mit.ctypes.data, cfd.ctypes.data, len(mit), float(threshold), str(method).encode(),
                            out.ctypes.data))
    return out
