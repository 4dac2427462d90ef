"""GPU parity at the edges of the batch verifiers' prepare and terms kernels (vrf_batch.hip) vs the oracle, bit for bit.

k_thin_prepare hashes a one-pair item of a 32-byte-point SHA-512 suite through a static layout up to the additional data and eight
bytes to a step after it (sha512_dev.h); every other item, also in the same wave, takes the general path.  k_thin_terms and
k_ped_terms hash the blocks of the weight stream once per workgroup of 256 items (batch_terms_dev.h WeightBlocks).

  additional-data lengths : where the challenge tail (44 + adl + 33 bytes into the second block on Bandersnatch) and the
                            delinearisation tail (44 + adl + 1) cross the 112-byte padding limit and the 128-byte block edge, once
                            and twice, every residue mod 8; uniform batches and all lengths mixed in one
  pair counts             : one-pair items between items with 0, 2, 3, 5, 16, 17 pairs; suites whose items never take the static
                            layout (33-byte points, SHA-256, SHAKE128)
  batch sizes             : around the workgroup of 256 items, the wave and the four items that share a block of the stream
  first index             : a shard that starts inside a block of the stream (avrf_*_batch_partial)"""
import ctypes as C
import random

import pytest

import oracle as orc
from helpers import nat_batch, xy

pytestmark = pytest.mark.gpu

ADLS = [0, 1, 2, 3, 4, 5, 7, 8, 13, 34, 35, 36, 50, 51, 52, 66, 67, 68, 83, 84, 85, 127, 128, 211, 212, 213, 300]
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
THIN, PEDERSEN = 0, 1
PROOF_LEN = {THIN: 96, PEDERSEN: 256}
RESP_OFF = {THIN: 64, PEDERSEN: 192}            # the response scalars: s (thin), s || sb (Pedersen)
TERMS_PER_ITEM = {THIN: 4, PEDERSEN: 5}         # one-pair items


class Contexts(dict):
    def __missing__(self, suite):
        from ark_vrf_amd import _native as nat
        self[suite] = nat.Context(suite)
        return self[suite]


@pytest.fixture(scope="module")
def ctxs():
    cs = Contexts()
    yield cs
    for c in cs.values():
        c.close()


# ---------------------------------------------------------------- one-pair items with a chosen additional data

_KEYS = {}


def key(suite, j):
    """(sk, pk, input, output) of item j, compressed, and their xy forms: made once, shared by every test"""
    if (suite, j) not in _KEYS:
        sk, pk = orc.from_seed(suite, bytes([j & 255, j >> 8, 77]) + bytes(29))
        h = orc.hash_to_curve(suite, b"layout-%d" % j)
        o = orc.vrf_output(suite, sk, h)
        _KEYS[suite, j] = (sk, pk, h, o, xy(suite, pk), xy(suite, h), xy(suite, o))
    return _KEYS[suite, j]


def one_pair_batch(suite, ad_lens):
    rng = random.Random(len(ad_lens) * 1000003 + sum(ad_lens))
    comp, abi = ([], [], [], []), ([], [], [], [])
    for j, adl in enumerate(ad_lens):
        sk, pk, h, o, pk_xy, h_xy, o_xy = key(suite, j)
        ad = rng.randbytes(adl)
        pr = orc.thin_prove(suite, sk, [(h, o)], ad)
        for dst, item in zip(comp, (pk, [(h, o)], ad, pr)):
            dst.append(item)
        for dst, item in zip(abi, (pk_xy, [(h_xy, o_xy)], ad, xy(suite, pr[:32]) + pr[32:])):
            dst.append(item)
    return comp, abi


def check_thin(c, suite, comp, abi, bad_item):
    assert c.thin_batch_verify(*abi) == 0
    st, bases, sc = orc.thin_batch_terms(suite, *comp)
    gb, gs = c.last_terms()
    assert st == 0 and gs == sc and gb == bases
    ads, proofs = list(abi[2]), list(abi[3])
    if ads[bad_item]:                                                         # one byte of the additional data ...
        ads[bad_item] = ads[bad_item][:-1] + bytes([ads[bad_item][-1] ^ 0x10])
    else:                                                                     # ... or, where there is none, of the response
        proofs[bad_item] = proofs[bad_item][:67] + bytes([proofs[bad_item][67] ^ 1]) + proofs[bad_item][68:]
    assert c.thin_batch_verify(abi[0], abi[1], ads, proofs) == 1


@pytest.mark.parametrize("adl", ADLS)
def test_additional_data_length_uniform(ctxs, adl):
    comp, abi = one_pair_batch(0, [adl] * 130)
    check_thin(ctxs[0], 0, comp, abi, 77)


def test_additional_data_lengths_mixed(ctxs):
    """every length in one batch of 192, shuffled: the position after the additional data differs from lane to lane"""
    lens = (ADLS * 8)[:192]
    random.Random(5).shuffle(lens)
    comp, abi = one_pair_batch(0, lens)
    check_thin(ctxs[0], 0, comp, abi, 100)


# ---------------------------------------------------------------- static-layout and general path in one wave

PAIRS = [0, 1, 2, 3, 1, 1, 17, 1, 5, 1, 1, 0, 2, 1, 16, 1, 1, 1, 3, 1]


@pytest.mark.parametrize("suite", [orc.BANDERSNATCH, orc.BABYJUBJUB, orc.BANDERSNATCH_SW, orc.BANDERSNATCH_SHAKE128, orc.TESTING_SHA256])
def test_pair_counts_in_one_wave(ctxs, suite):
    pks, ios, ads, proofs = [], [], [], []
    for j, m in enumerate(PAIRS):
        sk, pk = orc.from_seed(suite, bytes([j + 1, 9]) + bytes(30))
        io = []
        for i in range(m):
            h = orc.hash_to_curve(suite, b"wave-%d-%d" % (j, i))
            io.append((h, orc.vrf_output(suite, sk, h)))
        ad = b"ad%d" % j * (j % 7)
        pks.append(pk); ios.append(io); ads.append(ad); proofs.append(orc.thin_prove(suite, sk, io, ad))
    abi = ([xy(suite, p) for p in pks], [[(xy(suite, i), xy(suite, o)) for i, o in it] for it in ios], ads,
           [xy(suite, p[:32]) + p[32:] for p in proofs])
    c = ctxs[suite]
    assert c.thin_batch_verify(*abi) == 0
    st, bases, sc = orc.thin_batch_terms(suite, pks, ios, ads, proofs)
    gb, gs = c.last_terms()
    assert st == 0 and gs == sc and gb == bases
    for j in (3, 4):                                                          # a general-path item, a static-layout item
        bad = list(abi[3]); bad[j] = bad[j][:70] + bytes([bad[j][70] ^ 2]) + bad[j][71:]
        assert c.thin_batch_verify(abi[0], abi[1], abi[2], bad) == 1


# ---------------------------------------------------------------- synthetic batches: sizes and shards

_BATCHES = {}


def synthetic(suite, kind, n):
    if (suite, kind) not in _BATCHES:
        _BATCHES[suite, kind] = orc.gen_batch(suite, kind, 300)
    return items(_BATCHES[suite, kind], kind, 0, n)


def items(b, kind, lo, hi):
    """items [lo, hi) of a gen_batch dict (one pair per item)"""
    off = [0]
    for ln in b["ad_lens"]:
        off.append(off[-1] + ln)
    psz = PROOF_LEN[kind]
    return {"n": hi - lo, "sks": b["sks"][32 * lo: 32 * hi], "pks_xy": b["pks_xy"][64 * lo: 64 * hi], "ios_xy": b["ios_xy"][128 * lo: 128 * hi],
            "io_counts": b["io_counts"][lo: hi], "ads": b["ads"][off[lo]: off[hi]], "ad_lens": b["ad_lens"][lo: hi],
            "proofs": b["proofs"][psz * lo: psz * hi]}


def stage(c, kind, b):
    return c.thin_batch_stage(nat_batch(b)) if kind == THIN else c.pedersen_batch_stage(nat_batch(b))


def oracle_terms(suite, kind, b):
    return orc.thin_batch_terms_xy(suite, b) if kind == THIN else orc.pedersen_batch_terms_xy(suite, b)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("suite,kind", [(0, THIN), (1, THIN), (0, PEDERSEN)])
def test_workgroup_edges(ctxs, suite, kind, n):
    c, b = ctxs[suite], synthetic(suite, kind, n)
    run = c.thin_batch_run if kind == THIN else c.pedersen_batch_run
    assert stage(c, kind, b) == 0 and run() == 0
    st, bases, sc = oracle_terms(suite, kind, b)
    gb, gs = c.last_terms()
    assert st == 0 and gs == sc and gb == bases
    j = n // 2
    pr = bytearray(b["proofs"]); pr[PROOF_LEN[kind] * j + RESP_OFF[kind]] ^= 1
    assert stage(c, kind, dict(b, proofs=bytes(pr))) == 0 and run() == 1


@pytest.mark.parametrize("kind", [THIN, PEDERSEN])
def test_first_index(ctxs, kind):
    """A shard [k, k + 131) of a batch of 261 under the whole batch's weight seed: the scalars the shard builds are the oracle's for
    those items (the last term, the shard's share of the generator term, is its own)."""
    from ark_vrf_amd import _native as nat
    L, c, n, N = nat.lib(), ctxs[0], 131, 261
    challenges = L.avrf_thin_batch_challenges if kind == THIN else L.avrf_pedersen_batch_challenges
    partial = L.avrf_thin_batch_partial if kind == THIN else L.avrf_pedersen_batch_partial
    whole = synthetic(0, kind, N)
    psz, ro, per = PROOF_LEN[kind], RESP_OFF[kind], TERMS_PER_ITEM[kind]
    assert stage(c, kind, whole) == 0
    cs = (C.c_uint8 * (16 * N))()
    assert challenges(c._h, cs) == 0
    resp = b"".join(whole["proofs"][psz * j + ro: psz * (j + 1)] for j in range(N))
    seed, out = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    assert L.avrf_batch_weight_seed(0, kind, C.c_size_t(N), cs, nat._u8(resp), seed) == 0
    st, bases, sc = oracle_terms(0, kind, whole)
    assert st == 0
    for k in (1, 2, 3, 5, 130):
        shard = items(whole, kind, k, k + n)
        assert stage(c, kind, shard) == 0
        sub = (C.c_uint8 * (16 * n))()
        assert challenges(c._h, sub) == 0 and bytes(sub) == bytes(cs)[16 * k: 16 * (k + n)]
        assert partial(c._h, seed, C.c_uint64(k), out) == 0
        gb, gs = c.last_terms()
        assert gs[: 32 * per * n] == sc[32 * per * k: 32 * per * (k + n)], k
        assert gb[: 64 * per * n] == bases[64 * per * k: 64 * per * (k + n)], k
