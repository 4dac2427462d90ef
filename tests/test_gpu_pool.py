"""avrf_pool (include/avrf.h, csrc/pool.hip): many BatchVerifier::verify jobs in flight, native host threads, grouped weight
hashing, page-locked ingest.  Verdicts must be those of thin::BatchVerifier::verify (src/thin.rs:257-325) /
pedersen::BatchVerifier::verify (src/pedersen.rs:341-426), i.e. of the oracle and of the one-call entry points."""
import pytest

import oracle as orc
from helpers import IDENTITY_XY, nat_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from ark_vrf_amd import _native as nat
    return nat


def variants(suite, kind, n, seed):
    """a valid batch, one with a tampered response, one with a tampered proof point, (thin) one with an identity public key"""
    b = orc.gen_batch(suite, kind, n, start=100000 * seed)
    if kind == 1:
        b["pks_xy"] = b""
    psz = len(b["proofs"]) // n
    out = [b]
    pr = bytearray(b["proofs"]); pr[psz * (n // 2) + psz - 32] ^= 1
    out.append(dict(b, proofs=bytes(pr)))
    pr = bytearray(b["proofs"]); j = n - 1; pr[psz * j: psz * j + 64] = b["proofs"][psz * 0: psz * 0 + 64]     # another item's nonce point
    out.append(dict(b, proofs=bytes(pr)))
    if kind == 0:
        pk = bytearray(b["pks_xy"]); pk[64 * 3: 64 * 4] = bytes(64) if suite == 7 else IDENTITY_XY   # (short Weierstrass: the identity is all-zero)
        out.append(dict(b, pks_xy=bytes(pk)))
    return out


@pytest.mark.parametrize("suite,kind,group", [(0, 0, 1), (0, 0, 8), (0, 0, 16), (0, 1, 8), (1, 0, 16), (5, 0, 8), (5, 1, 1), (7, 0, 8)])
def test_pool_verdicts_match_oracle_and_one_call(nat, suite, kind, group):
    want_fn = orc.thin_batch_verify_xy if kind == 0 else orc.pedersen_batch_verify_xy
    bs = []
    for i, n in enumerate((300, 257, 64)):
        bs += variants(suite, kind, n, i)
    want = [want_fn(suite, b) for b in bs]
    assert 0 in want and 1 in want and (kind == 1 or 2 in want)
    c = nat.Context(suite)
    one_call = []
    for b in bs:
        stage = c.thin_batch_stage if kind == 0 else c.pedersen_batch_stage
        run = c.thin_batch_run if kind == 0 else c.pedersen_batch_run
        assert stage(nat_batch(b)) == 0
        one_call.append(run())
    c.close()
    assert one_call == want
    pool = nat.Pool(suite, kind=kind + 1, slots=5, lanes=2, threads=2, hash_group=group, depth=(1 if group == 1 else 0))
    try:
        nbs = [nat_batch(b) for b in bs]
        got = {}
        tickets = []
        for k, nb in enumerate(nbs):                                   # more batches than slots: submit blocks only while all are in flight
            if len(tickets) == 5:
                t0, k0 = tickets.pop(0)
                got[k0] = pool.wait(t0)
            tickets.append((pool.submit(nb), k))
        for t0, k0 in tickets:
            got[k0] = pool.wait(t0)
        assert [got[k] for k in range(len(bs))] == want
    finally:
        pool.close()


def test_pool_resubmit_cycle_and_pinned_ingest(nat):
    suite, n = 0, 1000
    good = orc.gen_batch(suite, 0, n)
    pr = bytearray(good["proofs"]); pr[96 * 11 + 64] ^= 1
    bad = dict(good, proofs=bytes(pr))
    assert orc.thin_batch_verify_xy(suite, good) == 0 and orc.thin_batch_verify_xy(suite, bad) == 1
    pool = nat.Pool(suite, kind=1, slots=6, lanes=3, threads=2, hash_group=8)
    try:
        def pinned(b):
            return nat.PinnedBatch(b["n"], b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=b["pks_xy"], proofs=b["proofs"])
        # the same batches from pageable and from page-locked buffers: same verdicts
        batches = [nat_batch(good), pinned(good), nat_batch(bad), pinned(bad), pinned(good), nat_batch(good)]
        tk = [pool.submit(b) for b in batches]
        assert [pool.wait(t) for t in tk] == [0, 0, 1, 1, 0, 0]
        # run the resident copies again, and stage them again from the host buffers
        tk2 = [pool.resubmit(t, from_host=(i % 2 == 1)) for i, t in enumerate(tk)]
        assert [pool.wait(t) for t in tk2] == [0, 0, 1, 1, 0, 0]
        with pytest.raises(nat.AvrfError):
            pool.wait(tk[0])                                           # a collected ticket is gone
        # cycle mode refuses mixed expectations: slots 2 and 3 hold the tampered batch
        done, mism, sec = pool.cycle(steps_block=6, min_seconds=0.0, expect=0)
        assert done == 6 and mism == 2 and sec > 0
        # make all six good (the resident tampered copies are overwritten), then whole blocks only
        tk3 = [pool.submit(b) for b in (batches[0], batches[1], batches[4], batches[5], batches[0], batches[1])]
        assert [pool.wait(t) for t in tk3] == [0] * 6
        for from_host in (False, True):
            done, mism, sec = pool.cycle(steps_block=7, min_seconds=0.05, from_host=from_host, expect=0)
            assert mism == 0 and done >= 7 and done % 7 == 0
        done, mism, sec = pool.cycle(steps_block=5, min_seconds=10.0, max_steps=20, expect=0)
        assert (done, mism) == (20, 0)
        st = pool.stats()
        assert st["hashed"] >= 6 and st["accumulate_launches"] >= 6 and st["cpu_us_hash"] > 0
    finally:
        pool.close()


def test_pool_empty_and_error_paths(nat):
    pool = nat.Pool(0, kind=1, slots=2, lanes=1, threads=1, hash_group=1)
    try:
        e = orc.gen_batch(0, 0, 0)
        assert pool.wait(pool.submit(nat_batch(e))) == 0               # src/thin.rs:262-264
        b = orc.gen_batch(0, 0, 40)
        t1, t2 = pool.submit(nat_batch(b)), pool.submit(nat_batch(b))
        import ctypes as C
        tk = C.c_uint64(0); nb = nat_batch(b)
        for _ in range(50):                                            # both slots hold uncollected verdicts: a third submit is refused
            import time; time.sleep(0.02)
        assert nat.lib().avrf_pool_submit(pool._h, C.c_size_t(nb.n), nb.pks_xy, nb.ios_xy, nb.io_counts, nb.ads, nb.ad_lens, nb.proofs, C.byref(tk)) == -2
        assert pool.wait(t2) == 0 and pool.wait(t1) == 0
        with pytest.raises(nat.AvrfError):
            pool.wait(12345)
        pool.set_validation(1)
        off = bytearray(b["ios_xy"]); off[5] ^= 0x40                   # an I/O point off the curve
        assert pool.wait(pool.submit(nat_batch(dict(b, ios_xy=bytes(off))))) == 2
    finally:
        pool.close()


def test_pool_concurrent_submitters_and_destroy_in_flight(nat):
    """several caller threads share one pool (submit / wait are thread-safe); a pool destroyed with work in flight shuts down cleanly"""
    import threading
    good = orc.gen_batch(0, 0, 400)
    pr = bytearray(good["proofs"]); pr[96 * 7 + 64] ^= 1
    bad = dict(good, proofs=bytes(pr))
    pool = nat.Pool(0, kind=1, slots=6, lanes=2, threads=2, hash_group=8)
    errs = []

    def caller(k):
        try:
            for i in range(6):
                b = bad if (k + i) % 3 == 0 else good
                want = 1 if (k + i) % 3 == 0 else 0
                got = pool.wait(pool.submit(nat_batch(b)))
                if got != want:
                    errs.append((k, i, got, want))
        except Exception as e:                                         # noqa: BLE001
            errs.append((k, repr(e)))
    th = [threading.Thread(target=caller, args=(k,)) for k in range(4)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not errs, errs
    # destroy with batches in flight: nothing to collect, no crash, a new pool works afterwards
    keep = [nat_batch(good) for _ in range(6)]
    for b in keep:
        pool.submit(b)
    pool.close()
    pool2 = nat.Pool(0, kind=1, slots=2, lanes=1, threads=1, hash_group=1)
    try:
        assert pool2.wait(pool2.submit(nat_batch(bad))) == 1
    finally:
        pool2.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_pool_full_size_batch(nat, kind):
    """BASELINE configs[1] / configs[2] size through the pool: 65 536 items (262 145 Thin terms / 327 682 Pedersen terms), a
    tampered copy next to the good one"""
    n = 65536
    good = orc.gen_batch(0, kind, n, threads=16)
    if kind == 1:
        good["pks_xy"] = b""
    psz = len(good["proofs"]) // n
    pr = bytearray(good["proofs"]); pr[psz * 40000 + psz - 26] ^= 2     # inside the last response scalar of item 40 000
    pool = nat.Pool(0, kind=kind + 1, slots=4, lanes=2, threads=2, hash_group=8)
    try:
        pg = nat.PinnedBatch(n, good["ios_xy"], good["io_counts"], good["ads"], good["ad_lens"], pks_xy=good["pks_xy"] or None, proofs=good["proofs"])
        tk = [pool.submit(pg), pool.submit(nat_batch(dict(good, proofs=bytes(pr)))), pool.submit(pg), pool.submit(pg)]
        assert [pool.wait(t) for t in tk] == [0, 1, 0, 0]
        done, mism, _ = pool.cycle(steps_block=8, min_seconds=0.0, expect=0)
        assert done == 8 and mism == 1                                  # eight runs over the four resident batches; the tampered slot is not reissued after its mismatch
    finally:
        pool.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_pool_wire_ingest(nat, kind):
    """avrf_pool_submit_wire: batches handed over as the reference's `serialize_compressed` bytes, decompressed and -- validate = 1 --
    checked as Validate::Yes does (src/lib.rs:410-433) on the device while they are staged.  Verdicts: valid 0, tampered scalar 1,
    a point that does not decode 2, a torsion point 2 under validate = 1 (and the equation's verdict under validate = 0);
    resubmission from the same host bytes; pinned and pageable sources; 65 536 items next to small batches."""
    import hashlib
    from helpers import compressed_items
    suite = 0
    q = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001

    def wire(b, n, pinned=False, pks=None, ios=None, proofs=None):
        p0, i0, ads, pr0 = compressed_items(suite, b, kind)
        pks = p0 if pks is None else pks; ios = i0 if ios is None else ios; proofs = pr0 if proofs is None else proofs
        cls = nat.PinnedBatch if pinned else nat.Batch
        return cls(n, b"".join(i + o for it in ios for i, o in it), [1] * n, b"".join(ads), [len(a) for a in ads],
                   pks_xy=(b"".join(pks) if kind == 0 else None), proofs=b"".join(proofs)), (pks, ios, ads, proofs)
    n = 300
    b = orc.gen_batch(suite, kind, n, start=7000)
    if kind == 1:
        b["pks_xy"] = b""
    good, (pks, ios, ads, proofs) = wire(b, n)
    j = n // 2
    tam = list(proofs); tam[j] = proofs[j][:-9] + bytes([proofs[j][-9] ^ 1]) + proofs[j][-8:]
    bad_y = next(k.to_bytes(32, "little") for k in range(2, 300) if orc.point_decompress(suite, k.to_bytes(32, "little"))[0] != 0)
    und = list(proofs); und[n - 1] = bad_y + proofs[n - 1][32:]
    st, oxy = orc.point_decompress(suite, ios[5][0][1])
    tors = orc.point_compress(suite, ((q - int.from_bytes(oxy[:32], "little")) % q).to_bytes(32, "little") + ((q - int.from_bytes(oxy[32:], "little")) % q).to_bytes(32, "little"))
    ios_t = list(ios); ios_t[5] = [(ios[5][0][0], tors)]
    pool = nat.Pool(suite, kind=kind + 1, slots=6, lanes=2, threads=2, hash_group=8)
    try:
        batches = [good, wire(b, n, pinned=True)[0], wire(b, n, proofs=tam)[0], wire(b, n, proofs=und)[0], wire(b, n, ios=ios_t)[0]]
        tk = [pool.submit_wire(x, validate=1) for x in batches]
        assert [pool.wait(t) for t in tk] == [0, 0, 1, 2, 2]
        tk = [pool.submit_wire(x, validate=0) for x in batches]
        got = [pool.wait(t) for t in tk]
        assert got[:4] == [0, 0, 1, 2] and got[4] in (0, 1)
        t2 = [pool.resubmit(t, from_host=True) for t in tk[:3]]                      # staged again from the same wire bytes
        assert [pool.wait(t) for t in t2] == [0, 0, 1]
        # a wire batch with a point that does not decode, run again from the slot's resident state: InvalidData again (not a bad-argument
        # error: the slot still holds that batch), and again after staging it from the host bytes once more
        t3 = pool.resubmit(tk[3], from_host=False)
        assert pool.wait(t3) == 2
        t4 = pool.resubmit(t3, from_host=True)
        assert pool.wait(t4) == 2
        assert pool.wait(pool.resubmit(t4, from_host=False)) == 2
        # a wire batch and an x || y batch side by side in one pool
        from helpers import nat_batch
        ta, tb = pool.submit_wire(good), pool.submit(nat_batch(b))
        assert (pool.wait(ta), pool.wait(tb)) == (0, 0)
        # full size
        N = 65536
        big = orc.gen_batch(suite, kind, N, threads=16)
        if kind == 1:
            big["pks_xy"] = b""
        gw, (_, _, _, bp) = wire(big, N, pinned=True)
        bt = list(bp); bt[40000] = bp[40000][:-9] + bytes([bp[40000][-9] ^ 1]) + bp[40000][-8:]
        tk = [pool.submit_wire(gw), pool.submit_wire(wire(big, N, proofs=bt)[0]), pool.submit_wire(gw, validate=0)]
        assert [pool.wait(t) for t in tk] == [0, 1, 0]
    finally:
        pool.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_pool_wire_ingest_host_weights(nat, golden_dir, kind):
    """avrf_pool_submit_wire on a suite whose weight transcript absorbs the responses on the host (5, Shake128Transcript): the wire
    staging takes them from behind the proof's compressed points.  The 7 reference vectors three times, the middle batch with a
    flipped response: verdicts 0 / 1 / 0, those of the one-call wire verifier, and the same again from the slots' resident state."""
    import ctypes as C
    import json
    import os
    suite = 5
    load = lambda k: json.load(open(os.path.join(golden_dir, f"bandersnatch_shake128_ell2_{k}.json")))
    th, pe = load("thin"), load("pedersen")
    pks = b"".join(bytes.fromhex(v["pk"]) for v in th)
    ios = b"".join(bytes.fromhex(v["h"] + v["gamma"]) for v in th)
    ads = [bytes.fromhex(v["ad"]) for v in th]
    if kind == 0:
        proofs = [bytes.fromhex(v["proof_r"] + v["proof_s"]) for v in th]
    else:
        proofs = [bytes.fromhex(v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"]) for v in pe]
    at = len(proofs[3]) - 20                                            # inside the last response scalar (s / sb) of item 3
    tam = proofs[:3] + [proofs[3][:at] + bytes([proofs[3][at] ^ 1]) + proofs[3][at + 1:]] + proofs[4:]
    wire = lambda pr: nat.Batch(7, ios, [1] * 7, b"".join(ads), [len(a) for a in ads], pks_xy=(pks if kind == 0 else None), proofs=b"".join(pr))
    batches = [wire(proofs), wire(tam), wire(proofs)]
    c = nat.Context(suite)
    one_call = []
    for b in batches:
        if kind == 0:
            one_call.append(nat.lib().avrf_thin_batch_verify_wire(c._h, C.c_size_t(7), b.pks_xy, b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, 1))
        else:
            one_call.append(nat.lib().avrf_pedersen_batch_verify_wire(c._h, C.c_size_t(7), b.ios_xy, b.io_counts, b.ads, b.ad_lens, b.proofs, 1))
    c.close()
    assert one_call == [0, 1, 0]
    pool = nat.Pool(suite, kind=kind + 1, slots=3, lanes=2, threads=2, hash_group=8)
    try:
        tk = [pool.submit_wire(b, validate=1) for b in batches]
        assert [pool.wait(t) for t in tk] == one_call
        tk = [pool.resubmit(t, from_host=False) for t in tk]
        assert [pool.wait(t) for t in tk] == one_call
    finally:
        pool.close()
