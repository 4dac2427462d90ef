"""GPU parity: the shared-table Pedersen batch staged from wire bytes (include/avrf.h avrf_pedersen_batch_stage_shared_wire), suites 0
and 4 (points of 32 and 33 bytes).

The expectation is always the x || y shared staging of the SAME batch (avrf_pedersen_batch_stage_shared), which run_and_compare pins to
the oracle's folded terms: the wire staging must leave, byte for byte, the same terms and the same verdict."""
import pytest

import oracle as orc
from helpers import IDENTITY_XY
from ped_shared_helpers import BAD_ARG, comp, nat_wire, point_len, prefix, real_batch, run_and_compare, shared, tampered, wire

pytestmark = pytest.mark.gpu

SUITES = [0, orc.BANDERSNATCH_SW]


@pytest.fixture(scope="module")
def ctxs():
    from ark_vrf_amd import _native as nat
    made = {}

    class Lazy(dict):
        def __missing__(self, suite):
            made[suite] = self[suite] = nat.Context(suite)
            return self[suite]
    yield Lazy()
    for c in made.values():
        c.close()


def same_as_xy(c, suite, sb, validate):
    """x || y shared staging (terms pinned to the oracle) -> wire staging of the same batch: same terms, same verdict; returns it"""
    st_xy = run_and_compare(c, suite, sb)
    want = c.last_terms()
    assert c.pedersen_batch_stage_shared_wire(nat_wire(suite, wire(suite, sb)), validate) == 0
    st = c.pedersen_batch_run()
    assert c.last_terms() == want
    assert st == st_xy
    return st


def bad_point(suite):
    """a y with no x on the curve, as tests/test_gpu_wire.py builds it (suite 0)"""
    return next(k.to_bytes(32, "little") for k in range(2, 300) if orc.point_decompress(suite, k.to_bytes(32, "little"))[0] != 0)


@pytest.mark.parametrize("validate", [0, 1])
@pytest.mark.parametrize("suite", SUITES)
def test_terms_equal_the_xy_flavour(ctxs, suite, validate):
    """130 one-pair items over 3 inputs: 3 + 130 + 390 points, so the rows, the outputs and the proofs' points each end inside a block"""
    assert SUITES == [0, 4] and ctxs[suite].point_len == point_len(suite) == 32 + (suite == 4)
    sb = real_batch(suite, [1] * 130, 3)
    assert same_as_xy(ctxs[suite], suite, sb, validate) == 0
    assert same_as_xy(ctxs[suite], suite, tampered(sb, 77, 224), validate) == 1


@pytest.mark.parametrize("suite", SUITES)
def test_mixed_pair_counts(ctxs, suite):
    """items without pairs have the identity as Ok: Validate::No only (validate != 0 refuses them, as the plain wire call does) and the
    32-byte encoding only (the identity has no 33-byte short-Weierstrass form that the decoder takes)"""
    c = ctxs[suite]
    if suite == 0:
        sb = real_batch(0, [0, 1, 2, 3, 16, 17, 1, 0], 4)
        assert same_as_xy(c, 0, sb, 0) == 0
        assert c.pedersen_batch_stage_shared_wire(nat_wire(0, wire(0, sb)), 1) == 2
    with_pairs = real_batch(suite, [1, 2, 17, 3, 1], 4)
    assert same_as_xy(c, suite, with_pairs, 1) == 0
    assert same_as_xy(c, suite, tampered(with_pairs, 2), 0) == 1


def test_rows_that_do_not_decode_and_identity_rows(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3)
    wb = wire(0, sb)
    before = tampered(sb, 2)
    ident = comp(0, IDENTITY_XY)
    for validate in (0, 1):
        for where, b in {"referenced row": dict(wb, rows=[wb["rows"][0], bad_point(0), wb["rows"][2]]),
                         "unreferenced row": dict(wb, rows=wb["rows"] + [bad_point(0)]),
                         "Ok": dict(wb, proofs=wb["proofs"][:19] + [wb["proofs"][19][:64] + bad_point(0) + wb["proofs"][19][96:]])}.items():
            assert c.pedersen_batch_stage_shared_wire(nat_wire(0, b), validate) == 2, where         # a row off the curve: AVRF_INVALID_DATA
            assert c.pedersen_batch_run() == BAD_ARG, where                                            # ... with nothing staged
            assert c.last_terms() == (b"", b"")
    spare = dict(wb, rows=wb["rows"] + [ident])                                                        # an identity row nothing refers to
    assert c.pedersen_batch_stage_shared_wire(nat_wire(0, spare), 0) == 0 and c.pedersen_batch_run() == 0      # validate = 0: it decodes
    assert c.last_terms()[0][64 * (4 * 20 + 3): 64 * (4 * 20 + 4)] == IDENTITY_XY
    idx = list(wb["input_index"]); idx[3] = 3
    assert c.pedersen_batch_stage_shared_wire(nat_wire(0, dict(spare, input_index=idx)), 0) == 0 and c.pedersen_batch_run() == 2   # referenced
    assert c.pedersen_batch_stage_shared_wire(nat_wire(0, spare), 1) == 2                              # validate = 1: refused though unreferenced
    # a bad index: refused on the host, the context keeps what it had staged
    assert same_as_xy(c, 0, before, 1) == 1
    idx = list(wb["input_index"]); idx[11] = 3
    assert c.pedersen_batch_stage_shared_wire(nat_wire(0, dict(wb, input_index=idx)), 1) == BAD_ARG
    assert c.pedersen_batch_run() == 1
    # the empty batch
    assert c.pedersen_batch_verify_shared_wire(nat_wire(0, shared([], [], [], [], [], [])), 1) == 0


@pytest.mark.parametrize("suite", SUITES)
def test_verify_call_equals_stage_and_run(ctxs, suite):
    c = ctxs[suite]
    sb = real_batch(suite, [1] * 130, 3)
    for b, verdict in [(sb, 0), (tampered(sb, 5), 1)]:
        nb = nat_wire(suite, wire(suite, b))
        assert c.pedersen_batch_stage_shared_wire(nb, 1) == 0 and c.pedersen_batch_run() == verdict
        want = c.last_terms()
        assert c.pedersen_batch_verify_shared_wire(nb, 1) == verdict
        assert c.last_terms() == want


@pytest.mark.parametrize("suite", SUITES)
def test_pool(suite):
    from ark_vrf_amd import _native as nat
    sb = real_batch(suite, [1] * 130, 3)
    wb = wire(suite, sb)
    good, bad = nat_wire(suite, wb), nat_wire(suite, wire(suite, tampered(sb, 5)))
    pool = nat.Pool(suite, device=0, kind=2, slots=2, lanes=1, threads=1)
    try:
        tk = [pool.submit_pedersen_shared_wire(good), pool.submit_pedersen_shared_wire(bad)]
        assert [pool.wait(t) for t in tk] == [0, 1]
        for from_host in (True, False):
            tk = [pool.resubmit(t, from_host=from_host) for t in tk]
            assert [pool.wait(t) for t in tk] == [0, 1]
        idx = list(wb["input_index"]); idx[129] = len(wb["rows"])
        with pytest.raises(nat.AvrfError):                                       # the indices are checked before a ticket exists
            pool.submit_pedersen_shared_wire(nat_wire(suite, dict(wb, input_index=idx)))
        if suite == 0:
            pr = list(wb["proofs"]); pr[129] = bad_point(0) + pr[129][32:]
            t = pool.submit_pedersen_shared_wire(nat_wire(0, dict(wb, proofs=pr)), validate=0)
            assert pool.wait(t) == 2
            t = pool.resubmit(t, from_host=False)                                # the resident state repeats the verdict
            assert pool.wait(t) == 2
    finally:
        pool.close()
    thin = nat.Pool(suite, device=0, kind=1, slots=1, lanes=1, threads=1)
    try:
        with pytest.raises(nat.AvrfError):
            thin.submit_pedersen_shared_wire(good)
    finally:
        thin.close()
