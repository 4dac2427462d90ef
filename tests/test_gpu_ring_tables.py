"""The ring prover's tables of all multiples as a per-setup resource (include/avrf.h avrf_ring_setup_set_table_budget /
build_tables / release_tables / tables): the widths an explicit budget plans, reported exactly; proofs on every planned width
equal to the reference's ring vectors byte for byte on both curves; the build / release lifecycle; two setups over one SRS;
and BN254 at the benchmark's ring-4096 shape on the tables."""
import gc
import hashlib
import json
import os

import pytest

import oracle as orc
from helpers import xy
from test_ring_table_plan import bases, plan, table_shape

pytestmark = pytest.mark.gpu
FILES = {0: ("bandersnatch_sha-512_ell2_ring.json", "bls12-381-srs-2-11-uncompressed-zcash.bin"),
         1: ("baby-jubjub_sha-512_tai_ring.json", "bn254-testing-2-9-uncompressed.bin")}
PAIRS = {0: [(10, 8), (12, 11), (14, 14)], 1: [(9, 8), (11, 10), (13, 13)]}   # (SRS c, witness c) at ring 8 (N = 512)
BATCH = 64                                                                      # the smallest prove call the tables serve


@pytest.fixture(scope="module")
def env(golden_dir):
    from ark_vrf_amd import _native as nat
    out = {}
    for suite, (vec, srsf) in FILES.items():
        out[suite] = (nat.Context(suite), open(os.path.join(golden_dir, srsf), "rb").read(), json.load(open(os.path.join(golden_dir, vec))))
    yield out
    for ctx, _, _ in out.values():
        ctx.close()


def ring_of(suite, v):
    raw = bytes.fromhex(v["ring_pks"])
    pks = [xy(suite, raw[32 * i: 32 * i + 32]) for i in range(len(raw) // 32)]
    return pks, pks.index(xy(suite, bytes.fromhex(v["pk"])))


def predicted(suite, c, kind):
    """(c, rows, bytes) tables() reports for a held table of width c (zeros for none)."""
    if not c:
        return (0, 0, 0)
    rows, _, nbytes = table_shape(1 if suite == 1 else 0, bases(suite, 8, kind), c)
    return (c, rows, nbytes)


def idle_bytes(ctx, srs):
    """Bytes of tables the process holds on the device before a test's own setups (normally 0)."""
    from ark_vrf_amd.ring import RingSetup
    gc.collect()
    s = RingSetup(ctx, srs, 8)
    b = s.tables()["process_bytes"]
    s.close()
    return b


def prove_vector(setup, suite, v, n=BATCH):
    pks, idx = ring_of(suite, v)
    key = setup.index(pks)
    assert key.commitment.hex() == v["ring_pks_com"]
    proofs = key.prove([idx] * n, [bytes.fromhex(v["blinding"])] * n)
    key.close()
    return proofs


@pytest.mark.parametrize("suite", [0, 1])
def test_budget_plans_and_proofs(env, suite):
    """Every budget: tables() reports exactly the planned (c, rows, bytes); 64 copies of each reference vector's proof are
    reproduced byte for byte, and the tables really served them (the counter rises), except at budget 0."""
    from ark_vrf_amd.ring import RingSetup, table_bytes
    ctx, srs, vs = env[suite]
    budgets = [table_bytes(suite, 8, 0, cs) + table_bytes(suite, 8, 1, cw) for cs, cw in PAIRS[suite]]
    budgets += [10**9, table_bytes(suite, 8, 0, 9 if suite else 10) - 1, 0]
    for budget in budgets:
        (pc, pb), (wc, wb) = plan(suite, 8, budget, table_bytes)
        setup = RingSetup(ctx, srs, 8)
        setup.set_table_budget(budget)
        assert setup.build_tables() == 0, budget
        t = setup.tables()
        assert t["srs"] == predicted(suite, pc, 0) and t["wit"] == predicted(suite, wc, 1), (budget, t)
        assert t["budget"] == budget and t["explicit"] and not t["missed"]
        assert t["state"] == (1 if pc else 0) | (2 if wc else 0) | 4 | (16 if budget == 0 else 0)
        for v in vs:
            before = setup.tables()["served"]
            assert prove_vector(setup, suite, v) == [bytes.fromhex(v["ring_proof"])] * BATCH
            after = setup.tables()["served"]
            assert (after == before) if budget == 0 else (after > before), (budget, before, after)
        setup.close()
    # the widths the issue names for these budgets
    assert [plan(suite, 8, b, table_bytes)[0][0] for b in budgets[:3]] == [p[0] for p in PAIRS[suite]]
    assert [plan(suite, 8, b, table_bytes)[1][0] for b in budgets[:3]] == [p[1] for p in PAIRS[suite]]
    if suite == 0:
        assert budgets[0] == 2_294_810_208 and plan(0, 8, 10**9, table_bytes) == ((0, 0), (9, table_bytes(0, 8, 1, 9)))


@pytest.mark.parametrize("suite", [0, 1])
def test_build_then_release_lifecycle(env, suite):
    from ark_vrf_amd.ring import RingSetup, table_bytes
    ctx, srs, vs = env[suite]
    v = vs[0]
    want = [bytes.fromhex(v["ring_proof"])] * BATCH
    base = idle_bytes(ctx, srs)
    cs, cw = PAIRS[suite][1]
    sizes = (table_bytes(suite, 8, 0, cs), table_bytes(suite, 8, 1, cw))
    setup = RingSetup(ctx, srs, 8)
    setup.set_table_budget(sum(sizes))
    assert setup.tables()["state"] == 4 and setup.tables()["process_bytes"] == base       # nothing before the build
    assert setup.build_tables() == 0
    t1 = setup.tables()
    assert t1["process_bytes"] == base + sum(sizes) and (t1["srs"][0], t1["wit"][0]) == (cs, cw)
    assert setup.build_tables() == 0 and setup.tables() == t1                           # the same plan again: a no-op
    # the first prove call after an explicit build builds nothing and runs on the tables
    assert prove_vector(setup, suite, v) == want
    t2 = setup.tables()
    assert t2["process_bytes"] == t1["process_bytes"] and t2["srs"] == t1["srs"] and t2["wit"] == t1["wit"]
    assert t2["served"] > t1["served"]
    # released: the memory goes back, and a batched call proves the same bytes on the bucket form without a lazy rebuild
    setup.release_tables()
    t3 = setup.tables()
    assert t3["process_bytes"] == base and t3["state"] == 4 and t3["srs"] == (0, 0, 0) == t3["wit"]
    assert prove_vector(setup, suite, v) == want
    t4 = setup.tables()
    assert t4["process_bytes"] == base and t4["served"] == t3["served"] and t4["state"] == 4
    # a new budget takes effect at the next build, which releases the old widths
    assert setup.build_tables() == 0 and setup.tables()["process_bytes"] == base + sum(sizes)
    cs2, cw2 = PAIRS[suite][0]
    sizes2 = (table_bytes(suite, 8, 0, cs2), table_bytes(suite, 8, 1, cw2))
    setup.set_table_budget(sum(sizes2))
    assert (setup.tables()["srs"][0], setup.tables()["wit"][0]) == (cs, cw)             # held until the next build
    assert setup.build_tables() == 0
    t5 = setup.tables()
    assert (t5["srs"][0], t5["wit"][0]) == (cs2, cw2) and t5["process_bytes"] == base + sum(sizes2)
    assert prove_vector(setup, suite, v) == want and setup.tables()["served"] > t5["served"]
    setup.close()
    assert idle_bytes(ctx, srs) == base


def test_default_budget_lazy_build_and_release(env, monkeypatch):
    """No explicit budget: the first 64-proof call builds within the process default (AVRF_RING_TABLE_GB, read at the build),
    as before; after release_tables the setup stays on the bucket form."""
    from ark_vrf_amd.ring import RingSetup
    ctx, srs, vs = env[0]
    v = vs[0]
    want = [bytes.fromhex(v["ring_proof"])] * BATCH
    monkeypatch.setenv("AVRF_RING_TABLE_GB", "3")
    monkeypatch.delenv("AVRF_RING_DIRECT", raising=False)
    gc.collect()
    setup = RingSetup(ctx, srs, 8)
    t0 = setup.tables()
    assert t0["state"] == 0 and t0["budget"] == 3 * 10**9
    assert prove_vector(setup, 0, v) == want
    t1 = setup.tables()
    assert t1["state"] & 1 and not t1["state"] & 4 and t1["served"] > 0
    assert t1["srs"][2] + t1["wit"][2] <= 3 * 10**9
    setup.release_tables()
    before = setup.tables()["served"]
    for _ in range(2):
        assert prove_vector(setup, 0, v) == want
        t2 = setup.tables()
        assert t2["state"] == 0 and t2["served"] == before and t2["srs"] == (0, 0, 0) == t2["wit"]
    setup.close()


def test_two_setups_share_or_hold_two_widths(env):
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup, table_bytes
    ctx, srs, vs = env[0]
    v = vs[1]
    want = [bytes.fromhex(v["ring_proof"])] * BATCH
    base = idle_bytes(ctx, srs)
    ctx2 = nat.Context(0)
    a, b = RingSetup(ctx, srs, 8), RingSetup(ctx2, srs, 8)
    (ca, cwa), (cb, cwb) = PAIRS[0][1], PAIRS[0][0]
    sa = table_bytes(0, 8, 0, ca) + table_bytes(0, 8, 1, cwa)
    sb = table_bytes(0, 8, 0, cb) + table_bytes(0, 8, 1, cwb)
    for s in (a, b):
        s.set_table_budget(sa)
        assert s.build_tables() == 0
    assert a.tables()["process_bytes"] == b.tables()["process_bytes"] == base + sa          # equal budgets: one copy, shared
    assert a.tables()["srs"] == b.tables()["srs"] and a.tables()["wit"] == b.tables()["wit"]
    b.set_table_budget(sb)
    assert b.build_tables() == 0
    assert b.tables()["process_bytes"] == base + sa + sb                                     # two widths of one SRS coexist
    assert (b.tables()["srs"][0], b.tables()["wit"][0]) == (cb, cwb)
    assert prove_vector(a, 0, v) == want and prove_vector(b, 0, v) == want
    b.close()
    assert a.tables()["process_bytes"] == base + sa                                          # freeing b freed only b's tables
    served = a.tables()["served"]
    assert prove_vector(a, 0, v) == want and a.tables()["served"] > served
    a.close()
    ctx2.close()
    assert idle_bytes(ctx, srs) == base


@pytest.mark.parametrize("suite", [0, 1])
def test_two_setups_back_to_back_then_commit_and_prove(env, suite):
    """Regression for the scratch race of commit d2e43ad (stream-ordered build scratch next to synchronous allocations: the first
    batched commitment after two setups on two streams came back as infinity): two setups created back to back on two contexts,
    tables built back to back, then both commit and prove."""
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup, table_bytes
    ctx, srs, vs = env[suite]
    v = vs[2]
    ctx2 = nat.Context(suite)
    a = RingSetup(ctx, srs, 8)
    b = RingSetup(ctx2, srs, 8)
    cs, cw = PAIRS[suite][0]
    for s in (a, b):
        s.set_table_budget(table_bytes(suite, 8, 0, cs) + table_bytes(suite, 8, 1, cw))
    assert a.build_tables() == 0 and b.build_tables() == 0
    pks, idx = ring_of(suite, v)
    ka, kb = a.index(pks), b.index(pks)
    assert ka.commitment.hex() == kb.commitment.hex() == v["ring_pks_com"]
    bl = bytes.fromhex(v["blinding"])
    for k in (ka, kb):
        assert k.prove([idx], [bl]) == [bytes.fromhex(v["ring_proof"])]
        assert k.prove([idx] * BATCH, [bl] * BATCH) == [bytes.fromhex(v["ring_proof"])] * BATCH
    ka.close(); kb.close(); a.close(); b.close(); ctx2.close()


def test_verifier_only_setup_has_no_tables(env):
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup
    ctx, srs, vs = env[0]
    full = RingSetup(ctx, srs, 8)
    vo = RingSetup(ctx, full.pcs_verifier_params(), 8, verifier_only=True)
    for call in (lambda: vo.set_table_budget(10**9), vo.build_tables, vo.release_tables, vo.tables):
        with pytest.raises(nat.AvrfError, match=f"-> {nat.SRS_LOOKUP_FAILED}$"):
            call()
    vo.close(); full.close()


def test_bn254_ring_4096_on_tables(golden_dir):
    """The benchmark's BN254 shape (ring 4096, N = 8192) on the tables: a budget of 130 GB plans (13, 8), and 64 copies of the
    oracle fixture's proof come out byte for byte and pass ring_batch_verify."""
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup, ring_batch_verify, srs_generate, table_bytes
    fx = json.load(open(os.path.join(golden_dir, "ring_large_oracle.json")))["bn254_ring4096"]
    suite, ring = fx["suite"], fx["ring_size"]
    r_bn = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
    srs_file = open(os.path.join(golden_dir, "bn254-testing-2-9-uncompressed.bin"), "rb").read()
    cnt = int.from_bytes(srs_file[:8], "little")
    g1, g2 = srs_file[8: 8 + 64], srs_file[8 + cnt * 64 + 8: 8 + cnt * 64 + 8 + 128]
    gc.collect()
    ctx = nat.Context(suite)
    urs = srs_generate(ctx, suite, int(fx["tau"], 16), g1, g2, ring)
    assert hashlib.sha256(urs).hexdigest() == fx["urs_sha256"]
    setup = RingSetup(ctx, urs, ring)
    budget = 130 * 10**9
    setup.set_table_budget(budget)
    assert setup.build_tables() == 0
    t = setup.tables()
    assert (t["srs"][0], t["wit"][0]) == (13, 8) and t["srs"][2] == table_bytes(1, 4096, 0, 13) == 122_564_122_688
    assert t["wit"][2] == table_bytes(1, 4096, 1, 8) and t["state"] == 1 | 2 | 4
    ks = b"".join((int.from_bytes(hashlib.sha512(b"k%d" % i).digest(), "little") % (r_bn >> 3) + 1).to_bytes(32, "little") for i in range(ring))
    pks_xy = ctx.scalar_mul_base(ks)
    pkl = [pks_xy[64 * i: 64 * i + 64] for i in range(ring)]
    key = setup.index(pkl)
    assert key.commitment.hex() == fx["commitment"]
    proofs = key.prove([fx["key_index"]] * BATCH, [bytes.fromhex(fx["blinding"])] * BATCH)
    assert proofs == [bytes.fromhex(fx["proof"])] * BATCH
    assert setup.tables()["served"] > t["served"]
    b = int.from_bytes(bytes.fromhex(fx["blinding"]), "little")
    st, bbxy = orc.point_decompress(suite, orc.smul(suite, b.to_bytes(32, "little"), orc.suite_point(suite, 1)))
    assert st == 0
    yb = ctx.msm(pkl[fx["key_index"]] + bbxy, (1).to_bytes(32, "little") * 2)
    assert ring_batch_verify(setup, [key.commitment], None, [yb] * BATCH, proofs) == 0
    key.close(); setup.close(); ctx.close()
