"""GPU: open batches (include/avrf.h avrf_*_batch_open / _push / avrf_batch_flush; BatchVerifier::new / push / verify, src/thin.rs:188-326,
src/pedersen.rs:303-426).  An open batch into which items were pushed in ANY chunking is indistinguishable from avrf_*_batch_stage of
the same items: every check compares the terms bit for bit and the verdict with the oracle's restatement of the reference and with a
one-shot stage + run of the same items on a second context."""
import json
import os

import pytest

import oracle as orc
from helpers import IDENTITY_XY, R_ORDER, proof_comp, proof_xy, xy

pytestmark = pytest.mark.gpu

THIN, PEDERSEN = 1, 2                      # ProofKind, as Context.batch_open takes it
OKIND = {THIN: 0, PEDERSEN: 1}             # the oracle's kind
PSZ = {THIN: 96, PEDERSEN: 256}
RESP = {THIN: 64, PEDERSEN: 192}           # where the responses start in an x || y proof
NAMES = {0: "bandersnatch_sha-512_ell2", 1: "baby-jubjub_sha-512_tai"}
BAD_ARG, INVALID = -2, 2                   # AVRF_ERR_BAD_ARG, AVRF_INVALID_DATA


class Contexts(dict):
    def __missing__(self, key):
        from ark_vrf_amd import _native as nat
        self[key] = nat.Context(key[0])
        return self[key]


@pytest.fixture(scope="module")
def ctxs():
    """ctxs[suite, 'open'] takes the pushes, ctxs[suite, 'shot'] the one-shot staging of the same items"""
    cs = Contexts()
    yield cs
    for c in cs.values():
        c.close()


class Items:
    """n items as per-item lists in the x || y forms of the C ABI (pks: None for Pedersen)"""

    def __init__(self, suite, kind, pks, ios, ads, proofs):
        self.suite, self.kind, self.pks, self.ios, self.ads, self.proofs = suite, kind, pks, ios, ads, proofs
        self.n = len(ads)

    @classmethod
    def from_gen(cls, suite, kind, b):
        n, off, ads = b["n"], 0, []
        for ln in b["ad_lens"]:
            ads.append(b["ads"][off: off + ln]); off += ln
        ios = [[(b["ios_xy"][128 * j: 128 * j + 64], b["ios_xy"][128 * j + 64: 128 * j + 128])] for j in range(n)]
        pks = [b["pks_xy"][64 * j: 64 * j + 64] for j in range(n)] if kind == THIN else None
        return cls(suite, kind, pks, ios, ads, [b["proofs"][PSZ[kind] * j: PSZ[kind] * (j + 1)] for j in range(n)])

    def but(self, **kw):
        """a copy with item j's field replaced: but(proofs=(j, value))"""
        f = dict(pks=self.pks, ios=self.ios, ads=self.ads, proofs=self.proofs)
        for name, (j, value) in kw.items():
            f[name] = list(f[name]); f[name][j] = value
        return Items(self.suite, self.kind, f["pks"], f["ios"], f["ads"], f["proofs"])

    def batch(self, lo=0, hi=None, wire=False):
        from ark_vrf_amd._native import Batch
        hi = self.n if hi is None else hi
        s, k = self.suite, OKIND[self.kind]
        pks, ios, proofs = self.pks and self.pks[lo:hi], self.ios[lo:hi], self.proofs[lo:hi]
        if wire:
            pks = pks and [orc.point_compress(s, p) for p in pks]
            ios = [[(orc.point_compress(s, i), orc.point_compress(s, o)) for i, o in it] for it in ios]
            proofs = [proof_comp(s, p, k) for p in proofs]
        return Batch.from_items(ios, self.ads[lo:hi], pks_xy=pks, proofs=proofs)

    def as_dict(self):
        return dict(n=self.n, pks_xy=b"".join(self.pks) if self.pks else b"", ios_xy=b"".join(i + o for it in self.ios for i, o in it),
                    io_counts=[len(it) for it in self.ios], ads=b"".join(self.ads), ad_lens=[len(a) for a in self.ads], proofs=b"".join(self.proofs))

    def oracle(self):
        """(status, bases, scalars) of the reference's batch MSM over all items"""
        return orc.thin_batch_terms_xy(self.suite, self.as_dict()) if self.kind == THIN else orc.pedersen_batch_terms_xy(self.suite, self.as_dict())


def run(c, kind):
    return c.thin_batch_run() if kind == THIN else c.pedersen_batch_run()


def one_shot(c, it):
    """avrf_*_batch_stage + run of all items: (status, terms)"""
    st = c.thin_batch_stage(it.batch()) if it.kind == THIN else c.pedersen_batch_stage(it.batch())
    assert st == 0
    st = run(c, it.kind)
    return st, c.last_terms()


def ranges(chunks):
    at = 0
    for n in chunks:
        yield at, at + n
        at += n


def push_all(c, it, chunks, wire=(), validate=1, hints=(0, 0, 0)):
    """open, then the items in `chunks` (wire: the indices of the chunks pushed as serialize_compressed bytes)"""
    assert sum(chunks) == it.n
    assert c.batch_open(it.kind, *hints) == 0
    for q, (lo, hi) in enumerate(ranges(chunks)):
        st = c.batch_push_wire(it.kind, it.batch(lo, hi, wire=True), validate) if q in wire else c.batch_push(it.kind, it.batch(lo, hi))
        assert st == 0, (q, st)
    pairs = sum(len(x) for x in it.ios)
    assert c.batch_pushed() == (it.n, pairs, sum(len(a) for a in it.ads))


def check_equivalent(ctxs, it, chunks, expect=0, oracle=True, **kw):
    """pushed in `chunks` == staged at once == the oracle: verdict, and for a batch that reaches its MSM the terms bit for bit"""
    co, cs = ctxs[it.suite, "open"], ctxs[it.suite, "shot"]
    push_all(co, it, chunks, **kw)
    st = run(co, it.kind)
    st1, terms1 = one_shot(cs, it)
    assert st == st1 == expect
    if expect != INVALID:
        assert co.last_terms() == terms1
        if oracle:
            sto, bases, sc = it.oracle()                                        # (the terms' status: 0 unless an item is InvalidData)
            assert sto == 0 and co.last_terms() == (bases, sc)
            verdict = orc.thin_batch_verify_xy if it.kind == THIN else orc.pedersen_batch_verify_xy
            assert verdict(it.suite, it.as_dict()) == expect
    return co


_GEN = {}


def gen(suite, kind, n):
    if (suite, kind, n) not in _GEN:
        _GEN[suite, kind, n] = Items.from_gen(suite, kind, orc.gen_batch(suite, OKIND[kind], n))
    return _GEN[suite, kind, n]


def tamper(p, at):
    return p[:at] + bytes([p[at] ^ 1]) + p[at + 1:]


# ---------------------------------------------------------------- the reference's vectors

def golden(golden_dir, suite, kind):
    load = lambda k: json.load(open(os.path.join(golden_dir, f"{NAMES[suite]}_{k}.json")))
    vs = load("thin" if kind == THIN else "pedersen")
    pks = [bytes.fromhex(v["pk"]) for v in vs]
    ios = [[(bytes.fromhex(v["h"]), bytes.fromhex(v["gamma"]))] for v in vs]
    ads = [bytes.fromhex(v["ad"]) for v in vs]
    if kind == THIN:
        proofs = [bytes.fromhex(v["proof_r"] + v["proof_s"]) for v in vs]
    else:
        proofs = [bytes.fromhex(v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"]) for v in vs]
    it = Items(suite, kind, [xy(suite, p) for p in pks] if kind == THIN else None, [[(xy(suite, i), xy(suite, o)) for i, o in x] for x in ios], ads,
               [proof_xy(suite, p, OKIND[kind]) for p in proofs])
    return it, (pks, ios, ads, proofs)


@pytest.mark.parametrize("suite", [0, 1])
@pytest.mark.parametrize("kind", [THIN, PEDERSEN])
def test_reference_vectors(ctxs, golden_dir, suite, kind):
    """the seven vectors pushed as 1 + 2 + 4: verdict 0, and the terms (29 for Thin) are the oracle's over the reference's own bytes"""
    it, (pks, ios, ads, proofs) = golden(golden_dir, suite, kind)
    c = check_equivalent(ctxs, it, [1, 2, 4])
    st, bases, sc = orc.thin_batch_terms(suite, pks, ios, ads, proofs) if kind == THIN else orc.pedersen_batch_terms(suite, ios, ads, proofs)
    assert st == 0 and c.last_terms() == (bases, sc) and len(sc) == 32 * (29 if kind == THIN else 37)


def test_empty_and_noop(ctxs):
    """an empty open batch verifies; a push of no items changes nothing"""
    from ark_vrf_amd._native import Batch
    for kind in (THIN, PEDERSEN):
        c = ctxs[0, "open"]
        assert c.batch_open(kind) == 0 and c.batch_pushed() == (0, 0, 0)
        assert c.batch_push(kind, Batch(0, b"", [], b"", [], pks_xy=b"", proofs=b"")) == 0
        assert c.batch_flush() == 0 and run(c, kind) == 0 and c.batch_pushed() == (0, 0, 0)


# ---------------------------------------------------------------- multi-pair items: pair offsets continue across chunks

@pytest.mark.parametrize("suite", [0, 1])
def test_multi_pair_items(ctxs, suite):
    """the ten items of test_multi_io_items (0, 1, 2, 3, 5, 1, 0, 2, 16, 17 pairs; 0 to 6 bytes of additional data) as 3 + 1 + 6 and as
    1 + 6 + 3, whose chunks end on the zero-pair items: the pair offsets continue across chunks, and the static-layout and the
    byte-wise prepare paths run within one chunk"""
    pks, ios, ads, proofs = [], [], [], []
    for j, m in enumerate([0, 1, 2, 3, 5, 1, 0, 2, 16, 17]):
        sk, pk = orc.from_seed(suite, bytes([j + 1]) + bytes(31))
        io = []
        for i in range(m):
            h = orc.hash_to_curve(suite, b"in-%d-%d" % (j, i))
            io.append((h, orc.vrf_output(suite, sk, h)))
        ad = b"ad%d" % j * (j % 3)
        pks.append(pk); ios.append(io); ads.append(ad); proofs.append(orc.thin_prove(suite, sk, io, ad))
    it = Items(suite, THIN, [xy(suite, p) for p in pks], [[(xy(suite, i), xy(suite, o)) for i, o in x] for x in ios], ads,
               [proof_xy(suite, p, 0) for p in proofs])
    c = check_equivalent(ctxs, it, [3, 1, 6])
    st, bases, sc = orc.thin_batch_terms(suite, pks, ios, ads, proofs)
    assert st == 0 and c.last_terms() == (bases, sc)
    # chunks that end on, and begin behind, the zero-pair items (0 and 6)
    check_equivalent(ctxs, it, [1, 6, 3])
    check_equivalent(ctxs, it.but(proofs=(3, tamper(it.proofs[3], 70))), [3, 1, 6], expect=1)


# ---------------------------------------------------------------- chunk sizes around the workgroup, growth, the Pippenger chain

EDGES = [(0, THIN, 600, [1, 127, 128, 129, 215]), (1, THIN, 300, [1, 127, 128, 44]), (0, PEDERSEN, 450, [1, 63, 129, 257])]


@pytest.mark.parametrize("suite,kind,n,chunks", EDGES)
def test_chunk_and_msm_edges(ctxs, suite, kind, n, chunks):
    """more than 2 048 terms on suite 0 (600 Thin items: 2 401, 450 Pedersen items: 2 252), chunks around the 128-thread workgroup of
    the prepare kernels, and all hints 0: every buffer grows, more than once"""
    check_equivalent(ctxs, gen(suite, kind, n), chunks)


def test_hints_and_growth_agree(ctxs):
    """exact hints, hints that are too small, and a context whose buffers an earlier, larger batch left: the same terms"""
    it = gen(0, THIN, 600)
    want = it.oracle()
    c = ctxs[0, "open"]
    for hints in [(600, 600, 24 * 600), (10, 3, 1), (0, 0, 0)]:
        push_all(c, it, [300, 300], hints=hints)
        assert run(c, THIN) == 0 and c.last_terms() == want[1:]


@pytest.mark.parametrize("suite", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("kind", [THIN, PEDERSEN])
def test_remaining_suites(ctxs, suite, kind):
    """sponge weights (5), SHA-256 (6, 7), the short-Weierstrass codec (4) and secp256r1 (7): 40 items as 1 + 39"""
    it = gen(suite, kind, 40)
    check_equivalent(ctxs, it, [1, 39])
    check_equivalent(ctxs, it.but(proofs=(20, tamper(it.proofs[20], RESP[kind]))), [1, 39], expect=1)


# ---------------------------------------------------------------- verify does not consume

@pytest.mark.parametrize("suite,kind", [(0, THIN), (0, PEDERSEN), (5, THIN)])
def test_verify_does_not_consume(ctxs, suite, kind):
    it = gen(suite, kind, 300 if kind == THIN and suite == 0 else 200)
    full = Items(suite, kind, it.pks and it.pks[:200], it.ios[:200], it.ads[:200], it.proofs[:200])
    co, cs = ctxs[suite, "open"], ctxs[suite, "shot"]
    assert co.batch_open(kind) == 0
    assert co.batch_push(kind, full.batch(0, 130)) == 0 and run(co, kind) == 0
    first = Items(suite, kind, it.pks and it.pks[:130], it.ios[:130], it.ads[:130], it.proofs[:130])
    assert co.last_terms() == one_shot(cs, first)[1]
    assert co.batch_push(kind, full.batch(130, 200)) == 0 and co.batch_pushed()[0] == 200
    assert run(co, kind) == 0
    assert co.last_terms() == one_shot(cs, full)[1] == full.oracle()[1:]
    # a tampered response in a later push fails the batch from then on; the earlier verdicts stood
    bad = full.but(proofs=(7, tamper(full.proofs[7], RESP[kind])))
    assert co.batch_push(kind, bad.batch(7, 8)) == 0
    assert run(co, kind) == 1 and run(co, kind) == 1
    assert co.batch_pushed()[0] == 201


# ---------------------------------------------------------------- defects: the one-shot's status

def test_defects(ctxs):
    it = gen(0, THIN, 300)
    chunks = [100, 100, 100]
    for j in (3, 150, 299):                                                   # a tampered response in the first, middle and last chunk
        check_equivalent(ctxs, it.but(proofs=(j, tamper(it.proofs[j], 64 + 5))), chunks, expect=1, oracle=False)
    check_equivalent(ctxs, it.but(pks=(120, IDENTITY_XY)), chunks, expect=INVALID)
    check_equivalent(ctxs, it.but(ios=(299, [(IDENTITY_XY, it.ios[299][0][1])])), chunks, expect=INVALID)
    check_equivalent(ctxs, it.but(ios=(0, [(it.ios[0][0][0], IDENTITY_XY)])), chunks, expect=INVALID)
    s_is_r = it.proofs[200][:64] + R_ORDER[0].to_bytes(32, "little")
    check_equivalent(ctxs, it.but(proofs=(200, s_is_r)), chunks, expect=INVALID)
    out_of_range = bytes([0xff] * 32) + it.pks[5][32:]
    check_equivalent(ctxs, it.but(pks=(5, out_of_range)), chunks, expect=INVALID)
    ad = it.ads[101]
    check_equivalent(ctxs, it.but(ads=(101, ad[:-1] + bytes([ad[-1] ^ 4]) if ad else b"x")), chunks, expect=1, oracle=False)
    # InvalidData is found at verify, not at push, and does not end the batch: the same verdict again
    co = ctxs[0, "open"]
    push_all(co, it.but(pks=(120, IDENTITY_XY)), chunks)
    assert co.batch_flush() == 0 and run(co, THIN) == INVALID and run(co, THIN) == INVALID
    ped = gen(0, PEDERSEN, 200)
    check_equivalent(ctxs, ped.but(proofs=(150, tamper(ped.proofs[150], 224))), [100, 100], expect=1, oracle=False)
    check_equivalent(ctxs, ped.but(proofs=(199, IDENTITY_XY + ped.proofs[199][64:])), [100, 100], expect=INVALID)


# ---------------------------------------------------------------- wire chunks

def test_wire_chunks(ctxs):
    it = gen(0, THIN, 600)
    chunks = [1, 127, 128, 129, 215]
    want = it.oracle()
    co = ctxs[0, "open"]
    push_all(co, it, chunks, wire=range(5))
    assert run(co, THIN) == 0 and co.last_terms() == want[1:]
    push_all(co, it, chunks, wire=(1, 3))                                      # wire and x || y chunks in one batch
    assert run(co, THIN) == 0 and co.last_terms() == want[1:]
    ped = gen(0, PEDERSEN, 200)
    push_all(co, ped, [70, 130], wire=(0, 1))
    assert run(co, PEDERSEN) == 0 and co.last_terms() == ped.oracle()[1:]


def test_wire_failure_is_sticky(ctxs):
    """an undecodable point in chunk 3: flush returns InvalidData, the batch is gone, a fresh open starts over"""
    from ark_vrf_amd._native import Batch
    it = gen(0, THIN, 300)
    co = ctxs[0, "open"]
    bad_y = next(k.to_bytes(32, "little") for k in range(2, 300) if orc.point_decompress(0, k.to_bytes(32, "little"))[0] != 0)
    assert co.batch_open(THIN) == 0
    for q, (lo, hi) in enumerate(ranges([100, 100, 100])):
        b = it.batch(lo, hi, wire=True)
        if q == 2:
            pks = bytearray(bytes(b.pks_xy)); pks[32 * 40: 32 * 41] = bad_y
            b = Batch(b.n, b.ios_xy, b.io_counts, b.ads, b.ad_lens, pks_xy=bytes(pks), proofs=b.proofs)
        assert co.batch_push_wire(THIN, b, 1) == 0                             # a push does not wait for its chunk's decoding
    assert co.batch_flush() == INVALID
    assert co.batch_pushed() == (0, 0, 0)
    assert co.thin_batch_run() == BAD_ARG and co.batch_flush() == BAD_ARG and co.batch_push(THIN, it.batch(0, 1)) == BAD_ARG
    # without a flush the next run reports it, and the batch is gone likewise
    assert co.batch_open(THIN) == 0
    b = it.batch(0, 100, wire=True)
    pks = bytearray(bytes(b.pks_xy)); pks[0:32] = bad_y
    assert co.batch_push_wire(THIN, Batch(b.n, b.ios_xy, b.io_counts, b.ads, b.ad_lens, pks_xy=bytes(pks), proofs=b.proofs), 0) == 0
    assert co.thin_batch_run() == INVALID and co.thin_batch_run() == BAD_ARG
    push_all(co, it, [100, 200], wire=(0,))
    assert run(co, THIN) == 0 and co.last_terms() == it.oracle()[1:]


# ---------------------------------------------------------------- the three-call run and segments

def test_three_call_run(ctxs):
    it = gen(0, THIN, 600)
    co = ctxs[0, "open"]
    push_all(co, it, [1, 127, 128, 129, 215])
    assert co.batch_run_begin() == 0 and co.batch_run_hash() == 0 and co.batch_run_end() == 0
    terms = co.last_terms()
    assert run(co, THIN) == 0 and co.last_terms() == terms == it.oracle()[1:]
    t = co.last_timing()
    assert t[0] > 0 and t[2] >= 0


@pytest.mark.parametrize("suite,kind,n,chunks,segs", [(0, THIN, 600, [1, 127, 128, 129, 215], [[1, 127, 300, 0, 172]]),
                                                      (0, PEDERSEN, 450, [1, 63, 129, 257], [[450], [200, 250]]),
                                                      (5, THIN, 40, [1, 39], [[13, 0, 27]])])
def test_segments(ctxs, suite, kind, n, chunks, segs):
    """avrf_*_batch_run_segments over the pushed items == the same call on the staged batch: statuses and every segment's terms"""
    it = gen(suite, kind, n)
    bad = it.but(proofs=(n - 3, tamper(it.proofs[n - 3], RESP[kind])))
    co, cs = ctxs[suite, "open"], ctxs[suite, "shot"]
    seg_run = (lambda c, s: c.thin_batch_run_segments(s)) if kind == THIN else (lambda c, s: c.pedersen_batch_run_segments(s))
    seg_terms = (lambda c, v: c.thin_segment_terms(v)) if kind == THIN else (lambda c, v: c.pedersen_segment_terms(v))
    for items, last in ((it, 0), (bad, 1)):
        push_all(co, items, chunks)
        assert (cs.thin_batch_stage(items.batch()) if kind == THIN else cs.pedersen_batch_stage(items.batch())) == 0
        for s in segs:
            got, want = seg_run(co, s), seg_run(cs, s)
            assert got == want == [0] * (len(s) - 1) + [last]
            for v in range(len(s)):
                assert seg_terms(co, v) == seg_terms(cs, v)
        assert run(co, kind) == last                                            # and the plain run of the same open batch afterwards
    assert seg_run(co, [n - 1]) == BAD_ARG                                      # counts that do not sum to what was pushed


# ---------------------------------------------------------------- refusals that change nothing; implicit close

def test_refusals(ctxs):
    from ark_vrf_amd import _native as nat
    it, ped = gen(0, THIN, 300), gen(0, PEDERSEN, 200)
    fresh = nat.Context(0)
    try:
        assert fresh.batch_push(THIN, it.batch(0, 5)) == BAD_ARG and fresh.batch_flush() == BAD_ARG            # nothing open
        assert fresh.thin_batch_stage(it.batch(0, 5)) == 0
        assert fresh.batch_push(THIN, it.batch(5, 9)) == BAD_ARG and fresh.batch_pushed() == (0, 0, 0)        # staged is not open
        assert fresh.thin_batch_run() == 0
    finally:
        fresh.close()
    co = ctxs[0, "open"]
    want = Items(0, THIN, it.pks[:200], it.ios[:200], it.ads[:200], it.proofs[:200]).oracle()[1:]

    def still_good():
        assert co.batch_pushed()[0] == 200 and run(co, THIN) == 0 and co.last_terms() == want

    push_all(co, Items(0, THIN, it.pks[:200], it.ios[:200], it.ads[:200], it.proofs[:200]), [77, 123])
    assert co.batch_push(PEDERSEN, ped.batch(0, 5)) == BAD_ARG                # the other kind
    still_good()
    assert co.batch_run_begin() == 0                                          # between run_begin and run_end
    assert co.batch_push(THIN, it.batch(200, 210)) == BAD_ARG and co.batch_flush() == BAD_ARG and co.batch_open(THIN) == BAD_ARG
    assert co.batch_run_hash() == 0 and co.batch_run_end() == 0 and co.last_terms() == want
    still_good()
    b = it.batch(200, 201)                                                    # a push that would pass the pair limit (0x1fffffff)
    over = nat.Batch(1, b.ios_xy, [0x1fffffff], b.ads, b.ad_lens, pks_xy=b.pks_xy, proofs=b.proofs)
    assert co.batch_push(THIN, over) == BAD_ARG
    nul = nat.Batch(1, b.ios_xy, b.io_counts, b.ads, b.ad_lens, pks_xy=None, proofs=b.proofs)              # no keys
    assert co.batch_push(THIN, nul) == BAD_ARG
    still_good()
    # whatever stages on the context ends the open batch
    assert co.thin_batch_stage(it.batch(0, 9)) == 0
    assert co.batch_pushed() == (0, 0, 0) and co.batch_push(THIN, it.batch(9, 12)) == BAD_ARG and co.batch_flush() == BAD_ARG
    assert co.thin_batch_run() == 0
    push_all(co, ped, [200])
    assert co.thin_verify(it.batch(0, 3)) == [0, 0, 0]                        # a per-item verifier likewise
    assert co.batch_push(PEDERSEN, ped.batch(0, 1)) == BAD_ARG


def test_close_with_chunks_queued(ctxs):
    """a staging call right behind many small pushes, nothing waited for in between: it ends the open batch, waits for the chunks
    still queued (they read the page-locked offsets it rewrites) and stages what it was given; likewise a new open"""
    it, ped = gen(0, THIN, 300), gen(0, PEDERSEN, 200)
    co = ctxs[0, "open"]
    few = Items(0, THIN, it.pks[250:], it.ios[250:], it.ads[250:], it.proofs[250:])
    for _ in range(3):
        assert co.batch_open(THIN) == 0
        for lo, hi in ranges([5] * 60):
            assert co.batch_push(THIN, it.batch(lo, hi)) == 0
        assert one_shot(co, few) == (0, few.oracle()[1:])                         # thin_batch_stage + run on the same context
        assert co.batch_pushed() == (0, 0, 0)
    assert co.batch_open(THIN) == 0
    for lo, hi in ranges([5] * 60):
        assert co.batch_push(THIN, it.batch(lo, hi)) == 0
    push_all(co, ped, [100, 100])                                                 # a new open of the other kind, at once
    assert run(co, PEDERSEN) == 0 and co.last_terms() == ped.oracle()[1:]


def test_invalid_item_segments_then_wire_push(ctxs):
    """an InvalidData item 0 in a segmented run (whose attribution pass writes per-item statuses) is not taken for a decode failure by
    a wire push behind it: the batch stays, with the statuses the staged batch gives"""
    it = gen(0, THIN, 300)
    bad = it.but(pks=(0, IDENTITY_XY))
    co, cs = ctxs[0, "open"], ctxs[0, "shot"]
    assert co.batch_open(THIN) == 0 and co.batch_push(THIN, bad.batch(0, 200)) == 0
    assert cs.thin_batch_stage(bad.batch(0, 200)) == 0
    assert co.thin_batch_run_segments([100, 100]) == cs.thin_batch_run_segments([100, 100]) == [INVALID, 0]
    assert co.batch_push_wire(THIN, bad.batch(200, 300, wire=True), 1) == 0
    assert co.batch_flush() == 0 and co.batch_pushed()[0] == 300
    assert cs.thin_batch_stage(bad.batch()) == 0
    assert co.thin_batch_run_segments([100, 100, 100]) == cs.thin_batch_run_segments([100, 100, 100]) == [INVALID, 0, 0]
    assert run(co, THIN) == INVALID and co.batch_pushed()[0] == 300


def test_validation_level_2(ctxs):
    """the context's own validation runs per chunk: a key outside the prime-order subgroup, the status the one-shot gives"""
    it = gen(0, THIN, 300)
    q = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    order2 = bytes(32) + (q - 1).to_bytes(32, "little")                       # (0, -1)
    bad = it.but(pks=(250, order2))
    co, cs = ctxs[0, "open"], ctxs[0, "shot"]
    try:
        co.set_validation(2); cs.set_validation(2)
        push_all(co, bad, [100, 100, 100])
        st = run(co, THIN)
        assert st == one_shot(cs, bad)[0] == INVALID
        check_equivalent(ctxs, it, [100, 100, 100])
    finally:
        co.set_validation(0); cs.set_validation(0)
    push_all(co, bad, [100, 100, 100])                                         # unchecked, the same key only fails the equation
    assert run(co, THIN) == one_shot(cs, bad)[0] == 1
