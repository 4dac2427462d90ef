"""A per-item call of more than ITEM_CHUNK = 131 072 items (capi.hip per_item_chunks) walks its items in chunks, launched back to
back: n = 131 075 through each of the six per-item entry points on suite 0.  The inputs are a 64-item oracle batch repeated
2048 times plus its first 3 items; the items are independent, so the expected outputs are the oracle's repeated the same way.
The tampered items sit on both sides of the chunk boundary: 131 071 is the last item of the first chunk, 131 073 the second
of the next."""
import pytest

import oracle as orc
from helpers import nat_batch

pytestmark = pytest.mark.gpu
BASE, REPS, TAIL = 64, 2048, 3
N = BASE * REPS + TAIL
BAD = (131071, 131073)


@pytest.fixture(scope="module")
def nat():
    from ark_vrf_amd import _native as nat
    return nat


def repeat(data, size):
    """the bytes of BASE items of `size` bytes each, repeated as the items are"""
    return data * REPS + data[: size * TAIL]


def repeated_batch(b, proofs, psz):
    return dict(b, n=N, sks=repeat(b["sks"], 32), pks_xy=repeat(b["pks_xy"], 64), ios_xy=repeat(b["ios_xy"], 128),
                io_counts=[1] * N, ads=b["ads"] * REPS + b["ads"][: sum(b["ad_lens"][:TAIL])],
                ad_lens=b["ad_lens"] * REPS + b["ad_lens"][:TAIL], proofs=repeat(proofs, psz))


def tampered(b, psz, s_off):
    pr = bytearray(b["proofs"])
    for j in BAD:
        pr[psz * j + s_off] ^= 1                                                   # a bit of the response scalar s
    return dict(b, proofs=bytes(pr))


def want_status():
    return [1 if j in BAD else 0 for j in range(N)]


def test_thin_prove_and_verify_across_the_chunk_boundary(nat):
    b = orc.gen_batch(0, 0, BASE)
    big = repeated_batch(b, b["proofs"], 96)
    c = nat.Context(0)
    try:
        assert c.thin_prove(nat_batch(big, with_sks=True, with_proofs=False)) == big["proofs"]
        assert c.thin_verify(nat_batch(tampered(big, 96, 64))) == want_status()
    finally:
        c.close()


def test_tiny_prove_and_verify_across_the_chunk_boundary(nat):
    b = orc.gen_batch(0, 0, BASE)
    proofs, off = [], 0
    for j in range(BASE):
        io = b["ios_xy"][128 * j: 128 * j + 128]
        ad = b["ads"][off: off + b["ad_lens"][j]]; off += b["ad_lens"][j]
        proofs.append(orc.tiny_prove(0, b["sks"][32 * j: 32 * j + 32], [(orc.point_compress(0, io[:64]), orc.point_compress(0, io[64:]))], ad))
    big = repeated_batch(b, b"".join(proofs), 48)
    c = nat.Context(0)
    try:
        assert c.tiny_prove(nat_batch(big, with_sks=True, with_proofs=False)) == big["proofs"]
        assert c.tiny_verify(nat_batch(tampered(big, 48, 16))) == want_status()
    finally:
        c.close()


def test_pedersen_prove_and_verify_across_the_chunk_boundary(nat):
    b = orc.gen_batch(0, 1, BASE)
    big = repeated_batch(b, b["proofs"], 256)
    c = nat.Context(0)
    try:
        pr, bl = c.pedersen_prove(nat_batch(b, with_sks=True, with_proofs=False))
        assert pr == b["proofs"]
        pr, bl_big = c.pedersen_prove(nat_batch(big, with_sks=True, with_proofs=False))
        assert pr == big["proofs"]
        assert bl_big == repeat(bl, 32)
        assert c.pedersen_verify(nat_batch(dict(tampered(big, 256, 192), pks_xy=b""))) == want_status()
    finally:
        c.close()
