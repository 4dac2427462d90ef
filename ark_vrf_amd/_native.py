"""ctypes binding of libavrf.so (the C ABI declared in include/avrf.h).

There is no CPU fallback: if the shared library is missing or no MI355X is visible, the
calls raise.  The library is built in-tree by `__graft_entry__.build()` /
`make -C ark_vrf_amd/csrc`.
"""
import ctypes as C
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AVRF_LIB_PATH") or os.path.join(_DIR, "libavrf.so")   # override: A/B builds of the same library

OK, VERIFICATION_FAILURE, INVALID_DATA, RING_CAPACITY_EXCEEDED, SRS_LOOKUP_FAILED = 0, 1, 2, 3, 4
ERR_NO_DEVICE, ERR_BAD_ARG = -1, -2

BANDERSNATCH_SHA512_ELL2 = 0
BABYJUBJUB_SHA512_TAI = 1
JUBJUB_SHA512_TAI = 2
ED25519_SHA512_TAI = 3          # Tiny / Thin / Pedersen only (no ring suite)
TESTING_SHA256_TAI = 6           # the crate's own test suite: edwards25519 with HashTranscript<Sha256> (no ring)
BANDERSNATCH_SHAKE128_ELL2 = 5   # suite 0's curve with the SHAKE128 sponge as transcript
SECP256R1_SHA256_TAI = 7        # NIST P-256, a genuinely short-Weierstrass suite (Tiny / Thin / Pedersen; no ring): 33-byte points, identity xy = zeros
BANDERSNATCH_SW_SHA512_TAI = 4  # Bandersnatch, short-Weierstrass presentation: 33-byte compressed points (Context.point_len)

THIN_PROOF_LEN = 96       # R_xy || s
PEDERSEN_PROOF_LEN = 256  # Yb_xy || R_xy || Ok_xy || s || sb


class AvrfError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AvrfError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.avrf_version.restype = C.c_char_p
        L.avrf_batch_last_terms.restype = C.c_size_t
        _lib = L
    return _lib


def _u8(data):
    if isinstance(data, C.Array):
        return data
    data = bytes(data)
    return (C.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(1, b"\0"))


def _u32(vals):
    if isinstance(vals, C.Array):
        return vals
    vals = list(vals)
    return (C.c_uint32 * max(1, len(vals)))(*vals)


def device_count():
    return lib().avrf_device_count()


def set_blocking_sync(device=0, on=True):
    """avrf_device_set_blocking_sync: waiting host threads sleep instead of spinning (device-wide)."""
    return lib().avrf_device_set_blocking_sync(int(device), 1 if on else 0)


class Batch:
    """Host-side packed batch in the C-ABI layout (see include/avrf.h)."""

    def __init__(self, n, ios_xy, io_counts, ads, ad_lens, pks_xy=None, proofs=None, sks=None):
        self.n = n
        self.ios_xy, self.io_counts, self.ads, self.ad_lens = _u8(ios_xy), _u32(io_counts), _u8(ads), _u32(ad_lens)
        self.pks_xy = _u8(pks_xy) if pks_xy is not None else None
        self.proofs = _u8(proofs) if proofs is not None else None
        self.sks = _u8(sks) if sks is not None else None

    @classmethod
    def from_items(cls, items_ios_xy, ads, pks_xy=None, proofs=None, sks=None):
        iob = b"".join(i + o for ios in items_ios_xy for i, o in ios)
        j = lambda v: None if v is None else b"".join(v)
        return cls(len(ads), iob, [len(x) for x in items_ios_xy], b"".join(ads), [len(a) for a in ads],
                   j(pks_xy), j(proofs), j(sks))


class SharedBatch:
    """A Thin batch over a table of shared points in the C-ABI layout (include/avrf.h avrf_thin_batch_stage_shared): shared_xy
    n_shared x 64, pk_index one row per item, input_index one row per I/O pair (item-major), outputs_xy one point per pair."""

    def __init__(self, n, shared_xy, pk_index, input_index, outputs_xy, io_counts, ads, ad_lens, proofs):
        self.n = n
        self.n_shared = len(shared_xy if isinstance(shared_xy, C.Array) else bytes(shared_xy)) // 64
        self.shared_xy, self.outputs_xy, self.ads, self.proofs = _u8(shared_xy), _u8(outputs_xy), _u8(ads), _u8(proofs)
        self.pk_index, self.input_index, self.io_counts, self.ad_lens = _u32(pk_index), _u32(input_index), _u32(io_counts), _u32(ad_lens)

    def args(self):
        return (C.c_size_t(self.n), C.c_size_t(self.n_shared), self.shared_xy, self.pk_index, self.input_index, self.outputs_xy,
                self.io_counts, self.ads, self.ad_lens, self.proofs)


def dedup_points(pks_xy, ios_xy):
    """An expanded batch's points -> (shared_xy, pk_index, input_index, outputs_xy): the byte-wise distinct rows among the public
    keys (n x 64) and the inputs (the first 64 of every 128 bytes of ios_xy), the row of every key and of every input, and the
    outputs on their own.  shared_xy[pk_index[j]] is item j's key again, shared_xy[input_index[k]] pair k's input."""
    import numpy as np
    pks = np.frombuffer(bytes(pks_xy), dtype=np.uint8).reshape(-1, 64)
    ios = np.frombuffer(bytes(ios_xy), dtype=np.uint8).reshape(-1, 128)
    pts = np.concatenate([pks, ios[:, :64]], axis=0)
    if not len(pts):
        return b"", [], [], b""
    rows, inverse = np.unique(pts, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    return (rows.tobytes(), [int(i) for i in inverse[: len(pks)]], [int(i) for i in inverse[len(pks):]],
            np.ascontiguousarray(ios[:, 64:]).tobytes())


class SharedWireBatch(SharedBatch):
    """A SharedBatch from wire bytes (include/avrf.h avrf_thin_batch_stage_shared_wire): `shared` n_shared x L and `outputs` one
    L-byte compressed point per pair, proofs n x (L + 32) laid out R || s; L = Context.point_len of the suite."""

    def __init__(self, n, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs, L=32):
        SharedBatch.__init__(self, n, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs)
        self.n_shared = len(shared if isinstance(shared, C.Array) else bytes(shared)) // L


def dedup_points_wire(pks, ios, L=32):
    """dedup_points on compressed points: pks n x L, ios pairs of L-byte points (input || output) -> (shared, pk_index,
    input_index, outputs), the rows being the byte-wise distinct compressed keys and inputs.  The encoding is canonical, so equal
    bytes <=> equal point."""
    import numpy as np
    pk = np.frombuffer(bytes(pks), dtype=np.uint8).reshape(-1, L)
    io = np.frombuffer(bytes(ios), dtype=np.uint8).reshape(-1, 2 * L)
    pts = np.concatenate([pk, io[:, :L]], axis=0)
    if not len(pts):
        return b"", [], [], b""
    rows, inverse = np.unique(pts, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    return (rows.tobytes(), [int(i) for i in inverse[: len(pk)]], [int(i) for i in inverse[len(pk):]],
            np.ascontiguousarray(io[:, L:]).tobytes())


def thin_shared_n_terms(n, tot_io, n_shared):
    """Terms of the MSM a shared-table Thin batch builds (host arithmetic; no device needed)."""
    f = lib().avrf_thin_shared_n_terms
    f.restype = C.c_size_t
    return f(C.c_size_t(n), C.c_size_t(tot_io), C.c_size_t(n_shared))


class PedersenSharedBatch:
    """A Pedersen batch over a table of shared inputs in the C-ABI layout (include/avrf.h avrf_pedersen_batch_stage_shared): shared_xy
    n_shared x 64, input_index one row per I/O pair (item-major), outputs_xy one point per pair, proofs n x 256."""

    def __init__(self, n, shared_xy, input_index, outputs_xy, io_counts, ads, ad_lens, proofs):
        self.n = n
        self.n_shared = len(shared_xy if isinstance(shared_xy, C.Array) else bytes(shared_xy)) // 64
        self.shared_xy, self.outputs_xy, self.ads, self.proofs = _u8(shared_xy), _u8(outputs_xy), _u8(ads), _u8(proofs)
        self.input_index, self.io_counts, self.ad_lens = _u32(input_index), _u32(io_counts), _u32(ad_lens)

    def args(self):
        return (C.c_size_t(self.n), C.c_size_t(self.n_shared), self.shared_xy, self.input_index, self.outputs_xy,
                self.io_counts, self.ads, self.ad_lens, self.proofs)


class PedersenSharedWireBatch(PedersenSharedBatch):
    """A PedersenSharedBatch from wire bytes (avrf_pedersen_batch_stage_shared_wire): `shared` n_shared x L and `outputs` one L-byte
    compressed point per pair, proofs n x (3 L + 64) laid out Yb || R || Ok || s || sb; L = Context.point_len of the suite."""

    def __init__(self, n, shared, input_index, outputs, io_counts, ads, ad_lens, proofs, L=32):
        PedersenSharedBatch.__init__(self, n, shared, input_index, outputs, io_counts, ads, ad_lens, proofs)
        self.n_shared = len(shared if isinstance(shared, C.Array) else bytes(shared)) // L


def dedup_inputs(ios_xy):
    """An expanded Pedersen batch's pairs -> (shared_xy, input_index, outputs_xy): the byte-wise distinct inputs (the first 64 of
    every 128 bytes of ios_xy), the row of every pair's input, and the outputs on their own.  No pairs: an empty table."""
    shared, _, input_index, outputs = dedup_points(b"", ios_xy)
    return shared, input_index, outputs


def dedup_inputs_wire(ios, L=32):
    """dedup_inputs on compressed points: ios pairs of L-byte points (input || output) -> (shared, input_index, outputs)."""
    shared, _, input_index, outputs = dedup_points_wire(b"", ios, L)
    return shared, input_index, outputs


def pedersen_shared_n_terms(n, n_shared):
    """Terms of the MSM a shared-table Pedersen batch builds, 4 n + n_shared + 2 (host arithmetic; no device needed)."""
    f = lib().avrf_pedersen_shared_n_terms
    f.restype = C.c_size_t
    return f(C.c_size_t(n), C.c_size_t(n_shared))


SEGMENT_TERMS_MAX, SEGMENTS_PADDED_TERMS_MAX, SEGMENTS_WINDOWS_MAX = 8191, 1 << 20, 65535   # include/avrf.h AVRF_SEGMENT*


def thin_segments_layout(seg_items, io_counts):
    """Layout of a segmented Thin run (host arithmetic; no device needed): seg_items items per segment over the items whose I/O pair
    counts are io_counts -> (L, padded terms, total terms, window bits), or ERR_BAD_ARG when the counts do not sum to
    len(io_counts) or a limit of include/avrf.h is exceeded."""
    seg_items, io_counts = list(seg_items), list(io_counts)
    out = (C.c_uint64 * 4)()
    st = lib().avrf_thin_segments_layout(C.c_size_t(len(io_counts)), C.c_size_t(len(seg_items)), _u32(seg_items), _u32(io_counts), out)
    return tuple(out) if st == OK else st


def pedersen_segments_layout(n, seg_items):
    """Layout of a segmented Pedersen run over n items (host arithmetic; no device needed; five terms per item and two per
    segment whatever the pair counts) -> (L, padded terms, total terms, window bits), or ERR_BAD_ARG as above."""
    seg_items = list(seg_items)
    out = (C.c_uint64 * 4)()
    st = lib().avrf_pedersen_segments_layout(C.c_size_t(n), C.c_size_t(len(seg_items)), _u32(seg_items), out)
    return tuple(out) if st == OK else st


def thin_shared_segments_layout(seg_items, io_counts, n_shared):
    """Layout avrf_thin_batch_run_shared_segments takes over a table of n_shared rows (host arithmetic; no device needed) ->
    (L, padded terms, total terms, window bits, mode) with mode 1 = merged, 0 = expanded, or ERR_BAD_ARG as thin_segments_layout."""
    seg_items, io_counts = list(seg_items), list(io_counts)
    out = (C.c_uint64 * 5)()
    st = lib().avrf_thin_shared_segments_layout(C.c_size_t(len(io_counts)), C.c_size_t(n_shared), C.c_size_t(len(seg_items)), _u32(seg_items),
                                                _u32(io_counts), out)
    return tuple(out) if st == OK else st


def pedersen_shared_segments_layout(n, seg_items, n_shared):
    """The same for avrf_pedersen_batch_run_shared_segments over n items and a table of n_shared inputs."""
    seg_items = list(seg_items)
    out = (C.c_uint64 * 5)()
    st = lib().avrf_pedersen_shared_segments_layout(C.c_size_t(n), C.c_size_t(n_shared), C.c_size_t(len(seg_items)), _u32(seg_items), out)
    return tuple(out) if st == OK else st


class Context:
    """One engine instance = suite + HIP stream + device workspace (avrf_ctx)."""

    thin_segments_layout = staticmethod(thin_segments_layout)
    pedersen_segments_layout = staticmethod(pedersen_segments_layout)
    thin_shared_segments_layout = staticmethod(thin_shared_segments_layout)
    pedersen_shared_segments_layout = staticmethod(pedersen_shared_segments_layout)

    def __init__(self, suite=BANDERSNATCH_SHA512_ELL2, device=0):
        self._h = C.c_void_p()
        st = lib().avrf_ctx_create(int(suite), int(device), C.byref(self._h))
        if st != OK:
            raise AvrfError(f"avrf_ctx_create failed with {st} (no MI355X visible? there is no CPU fallback)")
        self.suite = suite
        try:
            lib().avrf_point_len.restype = C.c_size_t
            self.point_len = lib().avrf_point_len(int(suite))  # serialize_compressed size of the suite's points: 32, or 33 (SW form)
        except AttributeError:                                 # an older build loaded through AVRF_LIB_PATH (A/B runs)
            self.point_len = 32

    def set_validation(self, level):
        """0: caller guarantees on-curve subgroup points (reference's typed-point contract); 1: on-curve check; 2: + subgroup."""
        st = lib().avrf_ctx_set_validation(self._h, int(level))
        if st != OK:
            raise AvrfError(f"avrf_ctx_set_validation -> {st}")

    def close(self):
        if self._h:
            lib().avrf_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- msm_unchecked
    def msm(self, bases_xy, scalars):
        n = len(scalars) // 32
        assert len(bases_xy) == 64 * n
        out = (C.c_uint8 * 64)()
        st = lib().avrf_msm_te(self._h, C.c_size_t(n), _u8(bases_xy), _u8(scalars), out)
        if st != OK:
            raise AvrfError(f"avrf_msm_te -> {st}")
        return bytes(out)

    def g1_msm(self, bases_xy, scalars):
        """KZG-side MSM on the suite's pairing curve; points as LE x||y (48+48 / 32+32 bytes)."""
        n = len(scalars) // 32
        fq = 48 if self.suite == 0 else 32
        assert len(bases_xy) == 2 * fq * n
        out = (C.c_uint8 * (2 * fq))()
        st = lib().avrf_g1_msm(self._h, C.c_size_t(n), _u8(bases_xy), _u8(scalars), out)
        if st != OK:
            raise AvrfError(f"avrf_g1_msm -> {st}")
        return bytes(out)

    def g1_msm_segments(self, n_seg, L, bases_xy, scalars):
        """n_seg independent G1 MSMs of L terms each as ONE chain (avrf_g1_msm_segments) -> list of n_seg points (LE x || y), or the
        refusal's status (ERR_BAD_ARG, INVALID_DATA)."""
        fq = 32 if int(self.suite) == 1 else 48          # BN254 for Baby-JubJub, BLS12-381 for every other suite with a pairing curve
        assert len(scalars) == 32 * n_seg * L and len(bases_xy) == 2 * fq * n_seg * L
        out = (C.c_uint8 * max(1, 2 * fq * n_seg))()
        st = lib().avrf_g1_msm_segments(self._h, C.c_size_t(n_seg), C.c_size_t(L), _u8(bases_xy), _u8(scalars), out)
        if st != OK:
            return st
        b = bytes(out)
        return [b[2 * fq * v: 2 * fq * (v + 1)] for v in range(n_seg)]

    # -- batch verifiers
    def thin_batch_verify(self, pks_xy, items_ios_xy, ads, proofs):
        b = Batch.from_items(items_ios_xy, ads, pks_xy=pks_xy, proofs=proofs)
        return lib().avrf_thin_batch_verify(self._h, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def thin_batch_stage(self, b):
        return lib().avrf_thin_batch_stage(self._h, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def thin_batch_stage_shared(self, b):
        """b: SharedBatch.  Staged for thin_batch_run / batch_run_begin .. / last_terms like a plain batch."""
        return lib().avrf_thin_batch_stage_shared(self._h, *b.args())

    def thin_batch_stage_shared_wire(self, b, validate=1):
        """b: SharedWireBatch.  INVALID_DATA when a row, an output or an R does not decode (validate: or fails Validate::Yes)."""
        return lib().avrf_thin_batch_stage_shared_wire(self._h, *b.args(), int(validate))

    def thin_batch_verify_shared_wire(self, b, validate=1):
        return lib().avrf_thin_batch_verify_shared_wire(self._h, *b.args(), int(validate))

    def thin_batch_run(self):
        return lib().avrf_thin_batch_run(self._h)

    def pedersen_batch_stage_shared(self, b):
        """b: PedersenSharedBatch.  Staged for pedersen_batch_run / batch_run_begin .. / last_terms like a plain batch."""
        return lib().avrf_pedersen_batch_stage_shared(self._h, *b.args())

    def pedersen_batch_stage_shared_wire(self, b, validate=1):
        """b: PedersenSharedWireBatch.  INVALID_DATA when a row, an output or a proof point does not decode (validate: or fails Validate::Yes)."""
        return lib().avrf_pedersen_batch_stage_shared_wire(self._h, *b.args(), int(validate))

    def pedersen_batch_verify_shared_wire(self, b, validate=1):
        return lib().avrf_pedersen_batch_verify_shared_wire(self._h, *b.args(), int(validate))

    # -- one verdict per segment of the staged Thin batch (include/avrf.h avrf_thin_batch_run_segments)
    def thin_batch_run_segments(self, seg_items):
        """seg_items: items per segment, consecutive, summing to the staged n -> list of statuses, or the refusal (ERR_BAD_ARG)."""
        return self._segments(seg_items, lib().avrf_thin_batch_run_segments)

    def thin_batch_verify_segments(self, b, seg_items):
        """stage + thin_batch_run_segments for a Batch."""
        return self._segments(seg_items, lib().avrf_thin_batch_verify_segments, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def thin_batch_verify_segments_wire(self, b, seg_items, validate=1):
        """The same for a Batch whose pks_xy / ios_xy / proofs fields hold the WIRE bytes (compressed points)."""
        return self._segments(seg_items, lib().avrf_thin_batch_verify_segments_wire, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens,
                              b.proofs, int(validate))

    # -- one verdict per segment of whatever Thin / Pedersen batch is staged, a shared-table one included (include/avrf.h
    # avrf_thin_batch_run_shared_segments): segment_terms afterwards are in the layout the run chose
    def thin_batch_run_shared_segments(self, seg_items):
        return self._segments(seg_items, lib().avrf_thin_batch_run_shared_segments)

    def pedersen_batch_run_shared_segments(self, seg_items):
        return self._segments(seg_items, lib().avrf_pedersen_batch_run_shared_segments)

    def thin_batch_verify_shared_segments_wire(self, b, seg_items, validate=1):
        """stage_shared_wire + thin_batch_run_shared_segments for a SharedWireBatch."""
        return self._segments(seg_items, lib().avrf_thin_batch_verify_shared_segments_wire, *b.args(), int(validate))

    def pedersen_batch_verify_shared_segments_wire(self, b, seg_items, validate=1):
        """stage_shared_wire + pedersen_batch_run_shared_segments for a PedersenSharedWireBatch."""
        return self._segments(seg_items, lib().avrf_pedersen_batch_verify_shared_segments_wire, *b.args(), int(validate))

    def _segments(self, seg_items, call, *args):
        """call(ctx, *args, n_seg, seg_items, status_out) -> the list of n_seg statuses, or the refusal."""
        seg_items = list(seg_items)
        out = (C.c_int32 * max(1, len(seg_items)))()
        st = call(self._h, *args, C.c_size_t(len(seg_items)), _u32(seg_items), out)
        return list(out)[: len(seg_items)] if st == OK else st

    def thin_segment_terms(self, seg):
        """(bases_xy, scalars) the last segmented run built for segment `seg`, as last_terms gives the plain run's."""
        return self._segment_terms(lib().avrf_thin_segment_terms, seg)

    # -- the same over the staged Pedersen batch (include/avrf.h avrf_pedersen_batch_run_segments)
    def pedersen_batch_run_segments(self, seg_items):
        """seg_items: items per segment, consecutive, summing to the staged n -> list of statuses, or the refusal (ERR_BAD_ARG)."""
        return self._segments(seg_items, lib().avrf_pedersen_batch_run_segments)

    def pedersen_batch_verify_segments(self, b, seg_items):
        """stage + pedersen_batch_run_segments for a Batch."""
        return self._segments(seg_items, lib().avrf_pedersen_batch_verify_segments, C.c_size_t(b.n), b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def pedersen_batch_verify_segments_wire(self, b, seg_items, validate=1):
        """The same for a Batch whose ios_xy / proofs fields hold the WIRE bytes (compressed points)."""
        return self._segments(seg_items, lib().avrf_pedersen_batch_verify_segments_wire, C.c_size_t(b.n), b.ios_xy, b.io_counts, b.ads, b.ad_lens,
                              b.proofs, int(validate))

    def pedersen_segment_terms(self, seg):
        """(bases_xy, scalars) the last segmented Pedersen run built for segment `seg`."""
        return self._segment_terms(lib().avrf_pedersen_segment_terms, seg)

    def _segment_terms(self, f, seg):
        f.restype = C.c_size_t
        k = f(self._h, C.c_size_t(seg), None, None)
        bases, sc = (C.c_uint8 * max(1, 64 * k))(), (C.c_uint8 * max(1, 32 * k))()
        assert f(self._h, C.c_size_t(seg), bases, sc) == k
        return bytes(bases)[: 64 * k], bytes(sc)[: 32 * k]

    def msm_segments(self, n_seg, bases_xy, scalars):
        """n_seg independent MSMs of L = len(scalars) / 32 / n_seg terms in one call -> list of n_seg result points (x || y)."""
        L = len(scalars) // 32 // n_seg if n_seg else 0
        assert len(scalars) == 32 * n_seg * L and len(bases_xy) == 64 * n_seg * L
        out = (C.c_uint8 * max(1, 64 * n_seg))()
        st = lib().avrf_msm_te_segments(self._h, C.c_size_t(n_seg), C.c_size_t(L), _u8(bases_xy), _u8(scalars), out)
        if st != OK:
            raise AvrfError(f"avrf_msm_te_segments -> {st}")
        return [bytes(out)[64 * v: 64 * v + 64] for v in range(n_seg)]

    def msm_segments_chain(self, n_seg, bases_xy, scalars, own_record=True):
        """msm_segments through the chain's two halves (avrf_msm_te_segments_chain, a test probe): one chain whatever n_seg is;
        own_record False: reported to a record of the call's own, as a pool slot's chain is."""
        L = len(scalars) // 32 // n_seg if n_seg else 0
        assert len(scalars) == 32 * n_seg * L and len(bases_xy) == 64 * n_seg * L
        out = (C.c_uint8 * max(1, 64 * n_seg))()
        st = lib().avrf_msm_te_segments_chain(self._h, C.c_size_t(n_seg), C.c_size_t(L), _u8(bases_xy), _u8(scalars), 1 if own_record else 0, out)
        if st != OK:
            raise AvrfError(f"avrf_msm_te_segments_chain -> {st}")
        return [bytes(out)[64 * v: 64 * v + 64] for v in range(n_seg)]

    def pedersen_batch_verify(self, items_ios_xy, ads, proofs):
        b = Batch.from_items(items_ios_xy, ads, proofs=proofs)
        return lib().avrf_pedersen_batch_verify(self._h, C.c_size_t(b.n), b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def pedersen_batch_stage(self, b):
        return lib().avrf_pedersen_batch_stage(self._h, C.c_size_t(b.n), b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def pedersen_batch_run(self):
        return lib().avrf_pedersen_batch_run(self._h)

    # the run of the staged batch in three calls (include/avrf.h): one host thread can keep several contexts in flight
    def batch_run_begin(self):
        return lib().avrf_batch_run_begin(self._h)

    def batch_run_hash(self):
        return lib().avrf_batch_run_hash(self._h)

    def batch_run_end(self):
        return lib().avrf_batch_run_end(self._h)

    # -- open batches (include/avrf.h avrf_*_batch_open): BatchVerifier::new, push as items arrive, then the run calls above
    def batch_open(self, kind, items_hint=0, pairs_hint=0, ad_bytes_hint=0):
        """kind: 1 Thin, 2 Pedersen.  An empty open batch on the context; the hints size its buffers (0: grow on demand)."""
        f = lib().avrf_thin_batch_open if kind == 1 else lib().avrf_pedersen_batch_open
        return f(self._h, C.c_size_t(items_hint), C.c_size_t(pairs_hint), C.c_size_t(ad_bytes_hint))

    def batch_push(self, kind, b):
        """b: a Batch, the chunk's items as x || y (a Thin chunk with pks_xy).  Returns at once: the chunk is copied, nothing is waited for."""
        n = C.c_size_t(b.n)
        if kind == 1:
            return lib().avrf_thin_batch_push(self._h, n, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)
        return lib().avrf_pedersen_batch_push(self._h, n, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def batch_push_wire(self, kind, b, validate=1):
        """The same for a Batch whose pks_xy / ios_xy / proofs fields hold the WIRE bytes.  A point that fails shows at the next push, flush or run."""
        n = C.c_size_t(b.n)
        if kind == 1:
            return lib().avrf_thin_batch_push_wire(self._h, n, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, int(validate))
        return lib().avrf_pedersen_batch_push_wire(self._h, n, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, int(validate))

    def batch_flush(self):
        """Waits for everything pushed and absorbs it; INVALID_DATA (and no batch) when a wire chunk did not decode."""
        return lib().avrf_batch_flush(self._h)

    def batch_pushed(self):
        """(items, pairs, bytes of additional data) pushed to the open batch so far; zeros when nothing is open."""
        out = (C.c_size_t * 3)()
        f = lib().avrf_batch_pushed
        f.restype = C.c_size_t
        n = f(self._h, out)
        assert n == out[0]
        return tuple(out)

    def last_terms(self):
        k = lib().avrf_batch_last_terms(self._h, None, None)
        bases, sc = (C.c_uint8 * max(1, 64 * k))(), (C.c_uint8 * max(1, 32 * k))()
        k2 = lib().avrf_batch_last_terms(self._h, bases, sc)
        assert k2 == k
        return bytes(bases)[: 64 * k], bytes(sc)[: 32 * k]

    def last_timing(self):
        out = (C.c_double * 8)()
        lib().avrf_last_timing(self._h, out)
        return list(out)

    # -- independent per-item calls
    def thin_prove(self, b):
        out = (C.c_uint8 * max(1, 96 * b.n))()
        st = lib().avrf_thin_prove(self._h, C.c_size_t(b.n), b.sks, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, out)
        if st != OK:
            raise AvrfError(f"avrf_thin_prove -> {st}")
        return bytes(out)[: 96 * b.n]

    def thin_verify(self, b):
        out = (C.c_int32 * max(1, b.n))()
        st = lib().avrf_thin_verify(self._h, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, out)
        if st != OK:
            raise AvrfError(f"avrf_thin_verify -> {st}")
        return list(out)[: b.n]

    def tiny_prove(self, b):
        out = (C.c_uint8 * max(1, 48 * b.n))()
        st = lib().avrf_tiny_prove(self._h, C.c_size_t(b.n), b.sks, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, out)
        if st != OK:
            raise AvrfError(f"avrf_tiny_prove -> {st}")
        return bytes(out)[: 48 * b.n]

    def tiny_verify(self, b):
        out = (C.c_int32 * max(1, b.n))()
        st = lib().avrf_tiny_verify(self._h, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, out)
        if st != OK:
            raise AvrfError(f"avrf_tiny_verify -> {st}")
        return list(out)[: b.n]

    def pedersen_prove(self, b):
        out, bl = (C.c_uint8 * max(1, 256 * b.n))(), (C.c_uint8 * max(1, 32 * b.n))()
        st = lib().avrf_pedersen_prove(self._h, C.c_size_t(b.n), b.sks, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, out, bl)
        if st != OK:
            raise AvrfError(f"avrf_pedersen_prove -> {st}")
        return bytes(out)[: 256 * b.n], bytes(bl)[: 32 * b.n]

    def pedersen_verify(self, b):
        out = (C.c_int32 * max(1, b.n))()
        st = lib().avrf_pedersen_verify(self._h, C.c_size_t(b.n), b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, out)
        if st != OK:
            raise AvrfError(f"avrf_pedersen_verify -> {st}")
        return list(out)[: b.n]

    # -- the same calls into caller-owned ctypes buffers (what a binding that keeps its buffers would do; no Python copies):
    # out: c_uint8 * (256 n) / (96 n); blindings: c_uint8 * (32 n) or None; status: c_int32 * n.  Return the call's status.
    def pedersen_prove_into(self, b, out, blindings=None):
        return lib().avrf_pedersen_prove(self._h, C.c_size_t(b.n), b.sks, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, out, blindings)

    def pedersen_verify_into(self, b, status):
        return lib().avrf_pedersen_verify(self._h, C.c_size_t(b.n), b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, status)

    def thin_prove_into(self, b, out):
        return lib().avrf_thin_prove(self._h, C.c_size_t(b.n), b.sks, b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, out)

    def thin_verify_into(self, b, status):
        return lib().avrf_thin_verify(self._h, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, status)

    def scalar_mul_base(self, scalars):
        n = len(scalars) // 32
        out = (C.c_uint8 * max(1, 64 * n))()
        st = lib().avrf_scalar_mul_base(self._h, C.c_size_t(n), _u8(scalars), out)
        if st != OK:
            raise AvrfError(f"avrf_scalar_mul_base -> {st}")
        return bytes(out)[: 64 * n]

    def scalar_mul(self, scalars, points_xy):
        n = len(scalars) // 32
        out = (C.c_uint8 * max(1, 64 * n))()
        st = lib().avrf_scalar_mul(self._h, C.c_size_t(n), _u8(scalars), _u8(points_xy), out)
        if st != OK:
            raise AvrfError(f"avrf_scalar_mul -> {st}")
        return bytes(out)[: 64 * n]

    def output_hash(self, points_xy, n_bytes=32):
        """Output::hash::<N> of output points given as x || y -> list of N-byte strings"""
        n = len(points_xy) // 64
        out = (C.c_uint8 * max(1, n_bytes * n))()
        st = lib().avrf_output_hash(self._h, C.c_size_t(n), _u8(points_xy), C.c_size_t(n_bytes), out)
        if st != OK:
            raise AvrfError(f"avrf_output_hash -> {st}")
        b = bytes(out)
        return [b[n_bytes * i: n_bytes * (i + 1)] for i in range(n)]

    def secret_from_seed(self, seeds, with_public=True):
        """Secret::from_seed for 32-byte seeds -> (secret scalars n x 32, public keys n x 64 or None)"""
        n = len(seeds) // 32
        sks = (C.c_uint8 * max(1, 32 * n))()
        pks = (C.c_uint8 * max(1, 64 * n))() if with_public else None
        st = lib().avrf_secret_from_seed(self._h, C.c_size_t(n), _u8(seeds), sks, pks)
        if st != OK:
            raise AvrfError(f"avrf_secret_from_seed -> {st}")
        return bytes(sks)[: 32 * n], (bytes(pks)[: 64 * n] if with_public else None)

    def hash_to_curve(self, messages):
        """Input::new for a list of byte strings -> (xy bytes n x 64, statuses)."""
        n = len(messages)
        out = (C.c_uint8 * max(1, n * 64))()
        st = (C.c_int32 * max(1, n))()
        rc = lib().avrf_hash_to_curve(self._h, C.c_size_t(n), _u8(b"".join(messages)), _u32([len(m) for m in messages]), out, st)
        if rc != OK:
            raise AvrfError(f"avrf_hash_to_curve -> {rc}")
        return bytes(out)[: n * 64], list(st)[:n]

    def points_decompress(self, comp, validate=False):
        n = len(comp) // self.point_len
        out, st_out = (C.c_uint8 * max(1, 64 * n))(), (C.c_int32 * max(1, n))()
        st = lib().avrf_points_decompress(self._h, C.c_size_t(n), _u8(comp), out, int(validate), st_out)
        if st != OK:
            raise AvrfError(f"avrf_points_decompress -> {st}")
        return bytes(out)[: 64 * n], list(st_out)[:n]

    def points_compress(self, xy):
        n = len(xy) // 64
        out = (C.c_uint8 * max(1, self.point_len * n))()
        st = lib().avrf_points_compress(self._h, C.c_size_t(n), _u8(xy), out)
        if st != OK:
            raise AvrfError(f"avrf_points_compress -> {st}")
        return bytes(out)[: self.point_len * n]


class PinnedBatch:
    """A Batch whose buffers live in page-locked host memory (avrf_host_alloc): staging copies from it are DMA transfers."""

    def __init__(self, n, ios_xy, io_counts, ads, ad_lens, pks_xy=None, proofs=None):
        self._pin_all(n, dict(ios_xy=ios_xy, ads=ads, pks_xy=pks_xy, proofs=proofs), dict(io_counts=io_counts, ad_lens=ad_lens))

    def _pin_all(self, n, byte_fields, u32_fields):
        """n and one pinned attribute per field (None stays None); the u32 fields are lists of counts or indices."""
        self.n = n
        self._ptrs = []
        for name, v in byte_fields.items():
            setattr(self, name, self._pin(bytes(v)) if v is not None else None)
        for name, v in u32_fields.items():
            setattr(self, name, self._pin(bytes(_u32(v))))

    def _pin(self, data):
        p = C.c_void_p()
        st = lib().avrf_host_alloc(C.c_size_t(max(1, len(data))), C.byref(p))
        if st != OK or not p:
            raise AvrfError(f"avrf_host_alloc -> {st}")
        C.memmove(p, data, len(data))
        self._ptrs.append(p)
        return p

    def close(self):
        for p in self._ptrs:
            lib().avrf_host_free(p)
        self._ptrs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedSharedBatch(PinnedBatch):
    """A SharedBatch whose buffers live in page-locked host memory."""

    def __init__(self, n, shared_xy, pk_index, input_index, outputs_xy, io_counts, ads, ad_lens, proofs):
        self.n_shared = len(bytes(shared_xy)) // 64
        self._pin_all(n, dict(shared_xy=shared_xy, outputs_xy=outputs_xy, ads=ads, proofs=proofs),
                      dict(pk_index=pk_index, input_index=input_index, io_counts=io_counts, ad_lens=ad_lens))

    args = SharedBatch.args


class PinnedSharedWireBatch(PinnedSharedBatch):
    """A SharedWireBatch whose buffers live in page-locked host memory."""

    def __init__(self, n, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs, L=32):
        PinnedSharedBatch.__init__(self, n, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs)
        self.n_shared = len(bytes(shared)) // L


class PinnedPedersenSharedBatch(PinnedBatch):
    """A PedersenSharedBatch whose buffers live in page-locked host memory."""

    def __init__(self, n, shared_xy, input_index, outputs_xy, io_counts, ads, ad_lens, proofs):
        self.n_shared = len(bytes(shared_xy)) // 64
        self._pin_all(n, dict(shared_xy=shared_xy, outputs_xy=outputs_xy, ads=ads, proofs=proofs),
                      dict(input_index=input_index, io_counts=io_counts, ad_lens=ad_lens))

    args = PedersenSharedBatch.args


class PinnedPedersenSharedWireBatch(PinnedPedersenSharedBatch):
    """A PedersenSharedWireBatch whose buffers live in page-locked host memory."""

    def __init__(self, n, shared, input_index, outputs, io_counts, ads, ad_lens, proofs, L=32):
        PinnedPedersenSharedBatch.__init__(self, n, shared, input_index, outputs, io_counts, ads, ad_lens, proofs)
        self.n_shared = len(bytes(shared)) // L


class Pool:
    """avrf_pool: many BatchVerifier::verify jobs in flight on one device (include/avrf.h).  kind 1 thin, 2 pedersen."""

    def __init__(self, suite=BANDERSNATCH_SHA512_ELL2, device=0, kind=1, slots=8, lanes=4, threads=2, hash_group=1, depth=0):
        self._h = C.c_void_p()
        st = lib().avrf_pool_create(int(suite), int(device), int(kind), int(slots), int(lanes), int(depth), int(threads), int(hash_group), C.byref(self._h))
        if st != OK:
            raise AvrfError(f"avrf_pool_create -> {st}")
        self.kind = kind
        self._keep = {}                                         # ticket -> batch object (its buffers must outlive the run)
        self._segs = {}                                         # segmented tickets -> number of segments

    def close(self):
        if self._h:
            lib().avrf_pool_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_validation(self, level):
        return lib().avrf_pool_set_validation(self._h, int(level))

    def _submit(self, symbol, b, *args):
        """One of the avrf_pool_submit* calls for batch object b -> the ticket; b is kept while the pool may read its buffers."""
        t = C.c_uint64(0)
        st = getattr(lib(), symbol)(self._h, *args, C.byref(t))
        if st != OK:
            raise AvrfError(f"{symbol} -> {st}")
        self._keep[t.value] = b
        return t.value

    def submit(self, b):
        """b: Batch or PinnedBatch.  Returns the ticket."""
        return self._submit("avrf_pool_submit", b, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs)

    def submit_shared(self, b):
        """b: SharedBatch (a kind 1 pool).  Returns the ticket."""
        return self._submit("avrf_pool_submit_shared", b, *b.args())

    def submit_shared_wire(self, b, validate=1):
        """b: SharedWireBatch / PinnedSharedWireBatch (a kind 1 pool).  Returns the ticket."""
        return self._submit("avrf_pool_submit_shared_wire", b, *b.args(), int(validate))

    def submit_pedersen_shared(self, b):
        """b: PedersenSharedBatch / PinnedPedersenSharedBatch (a kind 2 pool).  Returns the ticket."""
        return self._submit("avrf_pool_submit_pedersen_shared", b, *b.args())

    def submit_pedersen_shared_wire(self, b, validate=1):
        """b: PedersenSharedWireBatch / PinnedPedersenSharedWireBatch (a kind 2 pool).  Returns the ticket."""
        return self._submit("avrf_pool_submit_pedersen_shared_wire", b, *b.args(), int(validate))

    def submit_wire(self, b, validate=1):
        """b: a Batch / PinnedBatch whose pks_xy / ios_xy / proofs fields hold the WIRE bytes (compressed points)"""
        return self._submit("avrf_pool_submit_wire", b, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, int(validate))

    def submit_segments(self, b, seg_items):
        """A segmented job (avrf_pool_submit_segments): b as for submit, one verdict per run of seg_items[v] items.  Returns the ticket."""
        t = self._submit("avrf_pool_submit_segments", b, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs,
                         C.c_size_t(len(seg_items)), _u32(seg_items))
        self._segs[t] = len(seg_items)
        return t

    def submit_segments_wire(self, b, seg_items, validate=1):
        """The same from wire bytes (b as for submit_wire)."""
        t = self._submit("avrf_pool_submit_segments_wire", b, C.c_size_t(b.n), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs,
                         int(validate), C.c_size_t(len(seg_items)), _u32(seg_items))
        self._segs[t] = len(seg_items)
        return t

    def wait_segments(self, ticket, cap=None):
        """-> (status, statuses) of a segmented ticket: the job's status (the largest of its segments') and one status per segment, or
        None in their place when the job ended before any verdict (a staging error).  cap: room for that many statuses (default: the
        ticket's segments)."""
        unwritten = -(1 << 31)
        n_seg = self._segs.get(ticket, 0) if cap is None else int(cap)
        s, out = C.c_int(0), (C.c_int32 * max(1, n_seg))(*([unwritten] * max(1, n_seg)))
        st = lib().avrf_pool_wait_segments(self._h, C.c_uint64(ticket), C.byref(s), out, C.c_size_t(n_seg))
        if st != OK:
            raise AvrfError(f"avrf_pool_wait_segments -> {st}")
        got = list(out)[:n_seg]
        return s.value, (None if unwritten in got else got)

    def wait(self, ticket):
        s = C.c_int(0)
        st = lib().avrf_pool_wait(self._h, C.c_uint64(ticket), C.byref(s))
        if st != OK:
            raise AvrfError(f"avrf_pool_wait -> {st}")
        return s.value

    def resubmit(self, ticket, from_host=False):
        t = C.c_uint64(0)
        st = lib().avrf_pool_resubmit(self._h, C.c_uint64(ticket), 1 if from_host else 0, C.byref(t))
        if st != OK:
            raise AvrfError(f"avrf_pool_resubmit -> {st}")
        self._keep[t.value] = self._keep.pop(ticket, None)
        if ticket in self._segs:
            self._segs[t.value] = self._segs.pop(ticket)
        return t.value

    def cycle(self, steps_block, min_seconds=0.0, from_host=False, max_steps=0, expect=0):
        """-> (runs made, runs with another status than `expect`, seconds from first launch to last verdict)"""
        done, bad, sec = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        st = lib().avrf_pool_cycle(self._h, 1 if from_host else 0, C.c_uint64(steps_block), C.c_double(min_seconds), C.c_uint64(max_steps),
                                   int(expect), C.byref(done), C.byref(bad), C.byref(sec))
        if st != OK:
            raise AvrfError(f"avrf_pool_cycle -> {st}")
        return done.value, bad.value, sec.value

    def stats(self, reset=False):
        out = (C.c_double * 16)()
        st = lib().avrf_pool_stats(self._h, 1 if reset else 0, out, C.c_size_t(16))
        if st != OK:
            raise AvrfError(f"avrf_pool_stats -> {st}")
        k = ["cpu_us_begin", "cpu_us_collect", "cpu_us_hash", "cpu_us_launch", "cpu_us_end", "cpu_us_total", "hash_groups", "hashed", "sleeps",
             "accumulate_ms_total", "accumulate_launches"]
        return {k[i]: out[i] for i in range(len(k))}
