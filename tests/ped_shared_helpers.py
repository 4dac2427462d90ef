"""Helpers of the shared-table Pedersen tests (include/avrf.h avrf_pedersen_batch_stage_shared): batches as dicts, the expanded batch,
the oracle's terms folded into the shared layout, and material made once per process by the oracle's prover.

A shared Pedersen batch is a dict: rows (list of 64-byte x || y points), input_index (one row per I/O pair, item-major), outputs (list
of 64-byte points), io_counts, ads (list), proofs (list of 256 bytes: Yb || R || Ok || s || sb)."""
import random
from concurrent.futures import ThreadPoolExecutor

import oracle as orc
from helpers import IDENTITY_XY, R_ORDER, xy

Q = {0: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
     1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
BAD_ARG = -2


def shared(rows, input_index, outputs, io_counts, ads, proofs):
    assert len(io_counts) == len(ads) == len(proofs) and len(input_index) == len(outputs) == sum(io_counts)
    return dict(n=len(io_counts), rows=list(rows), input_index=list(input_index), outputs=list(outputs), io_counts=list(io_counts),
                ads=list(ads), proofs=list(proofs))


def nat_shared(sb):
    from ark_vrf_amd._native import PedersenSharedBatch
    return PedersenSharedBatch(sb["n"], b"".join(sb["rows"]), sb["input_index"], b"".join(sb["outputs"]), sb["io_counts"],
                               b"".join(sb["ads"]), [len(a) for a in sb["ads"]], b"".join(sb["proofs"]))


def expanded(sb):
    """the plain batch a shared one stands for, in the C-ABI layout (a gen_batch-style dict)"""
    rows = sb["rows"]
    return dict(n=sb["n"], pks_xy=b"", ios_xy=b"".join(rows[r] + o for r, o in zip(sb["input_index"], sb["outputs"])),
                io_counts=sb["io_counts"], ads=b"".join(sb["ads"]), ad_lens=[len(a) for a in sb["ads"]], proofs=b"".join(sb["proofs"]), sks=b"")


def prefix(sb, n):
    tot = sum(sb["io_counts"][:n])
    return shared(sb["rows"], sb["input_index"][:tot], sb["outputs"][:tot], sb["io_counts"][:n], sb["ads"][:n], sb["proofs"][:n])


def flip(data, at):
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


def tampered(sb, j, at=192):
    """the lowest bit of byte `at` of item j's proof: 192 is s, 224 sb, 128 the x of Ok"""
    pr = list(sb["proofs"])
    pr[j] = flip(pr[j], at)
    return dict(sb, proofs=pr)


def check_terms(suite, sb, got):
    """The device's terms (bases, scalars) of shared batch sb against the oracle's pedersen_batch_terms_xy of the EXPANDED batch, folded
    here: item terms O, Ok, Yb, R at 4 j + {0, 1, 2, 3} and the two base terms bit for bit; the row bases bit for bit; the row scalars
    bit for bit -- the sum mod r of the (I, -t s) scalars of the items that reference the row -- when no item has more than one pair,
    else (the oracle has no z_i) as a group element: msm of the T row terms == msm of the oracle's n merged-input terms, not the identity."""
    from ark_vrf_amd import _native as nat
    gb, gs = got
    n, rows, counts, r_order = sb["n"], sb["rows"], sb["io_counts"], R_ORDER[suite]
    t = len(rows)
    st_o, bases, sc = orc.pedersen_batch_terms_xy(suite, expanded(sb))
    assert st_o == 0 and len(sc) == 32 * (5 * n + 2)
    assert len(gs) // 32 == len(gb) // 64 == 4 * n + t + 2 == nat.pedersen_shared_n_terms(n, t)
    term = lambda k: (bases[64 * k: 64 * k + 64], sc[32 * k: 32 * k + 32])
    dev = lambda k: (gb[64 * k: 64 * k + 64], gs[32 * k: 32 * k + 32])
    for j in range(n):
        for at, k in enumerate((0, 1, 3, 4)):
            assert dev(4 * j + at) == term(5 * j + k), (j, k)
    assert dev(4 * n + t) == term(5 * n) and dev(4 * n + t + 1) == term(5 * n + 1)
    assert gb[64 * 4 * n: 64 * (4 * n + t)] == b"".join(rows)
    row_sc = gs[32 * 4 * n: 32 * (4 * n + t)]
    if max(counts, default=0) <= 1:
        acc, io0 = [0] * t, 0
        for j, m in enumerate(counts):
            if m:
                ib, is_ = term(5 * j + 2)
                assert ib == rows[sb["input_index"][io0]]
                acc[sb["input_index"][io0]] += int.from_bytes(is_, "little")
            io0 += m
        assert row_sc == b"".join((a % r_order).to_bytes(32, "little") for a in acc)
    else:
        want = orc.msm(suite, b"".join(term(5 * j + 2)[0] for j in range(n)), b"".join(term(5 * j + 2)[1] for j in range(n)))
        assert want != IDENTITY_XY                                                    # a partial sum: not vacuous
        assert orc.msm(suite, b"".join(rows), row_sc) == want
    referenced = set(sb["input_index"])
    for r in range(t):
        if r not in referenced:
            assert row_sc[32 * r: 32 * r + 32] == bytes(32), r


def run_and_compare(c, suite, sb):
    """stage shared, run, compare all terms with the oracle's; returns the verdict"""
    assert c.pedersen_batch_stage_shared(nat_shared(sb)) == 0
    st = c.pedersen_batch_run()
    check_terms(suite, sb, c.last_terms())
    return st


_REAL = {}


def real_batch(suite, counts, n_inputs, seed=1):
    """a VERIFYING batch of len(counts) items with counts[j] pairs each over n_inputs inputs and 5 keys: proofs by the oracle's prover.
    The table is the n_inputs inputs."""
    key = (suite, tuple(counts), n_inputs, seed)
    if key in _REAL:
        return _REAL[key]
    L = orc.pt_len(suite)
    rng = random.Random(seed)
    keys = [orc.from_seed(suite, bytes([k + 1, seed]) + bytes(30)) for k in range(5)]
    inputs = [orc.hash_to_curve(suite, b"ticket-%d" % i) for i in range(n_inputs)]
    outs = {(k, i): orc.vrf_output(suite, keys[k][0], inputs[i]) for k in range(5) for i in range(n_inputs)}
    plan = [(rng.randrange(5), [rng.randrange(n_inputs) for _ in range(m)], b"ad-%d" % j * (j % 3)) for j, m in enumerate(counts)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        proofs = list(ex.map(lambda p: orc.pedersen_prove(suite, keys[p[0]][0], [(inputs[i], outs[p[0], i]) for i in p[1]], p[2])[0], plan))
    out_xy = {ki: xy(suite, o) for ki, o in outs.items()}
    sb = shared([xy(suite, h) for h in inputs], [i for _, ii, _ in plan for i in ii], [out_xy[k, i] for k, ii, _ in plan for i in ii],
                counts, [ad for _, _, ad in plan], [b"".join(xy(suite, p[L * k: L * k + L]) for k in range(3)) + p[3 * L:] for p in proofs])
    _REAL[key] = sb
    return sb


def real3k():
    return real_batch(0, [1] * 3000, 3)


def torsion(suite, pxy):
    """(x, y) -> (-x, -y), as tests/test_gpu_wire.py::test_torsion_points builds it: on the curve, outside the prime-order subgroup"""
    q = Q[suite]
    return ((q - int.from_bytes(pxy[:32], "little")) % q).to_bytes(32, "little") + ((q - int.from_bytes(pxy[32:], "little")) % q).to_bytes(32, "little")


# ---- wire forms

_COMP = {}


def comp(suite, pxy):
    """x || y -> the suite's wire point (suite 4: the oracle's 32-byte form re-encoded as the 33-byte short-Weierstrass one)"""
    key = (suite, pxy)
    if key not in _COMP:
        w = orc.point_compress(suite, pxy)
        _COMP[key] = orc.sw_encode(suite, w) if suite == orc.BANDERSNATCH_SW else w
    return _COMP[key]


def point_len(suite):
    return 33 if suite == orc.BANDERSNATCH_SW else orc.pt_len(suite)


def wire(suite, sb):
    """the batch's wire form: rows / outputs as lists of compressed points, proofs as Yb || R || Ok || s || sb"""
    return dict(sb, rows=[comp(suite, r) for r in sb["rows"]], outputs=[comp(suite, o) for o in sb["outputs"]],
                proofs=[b"".join(comp(suite, p[64 * k: 64 * k + 64]) for k in range(3)) + p[192:] for p in sb["proofs"]])


def nat_wire(suite, wb):
    from ark_vrf_amd._native import PedersenSharedWireBatch
    L = point_len(suite)
    assert all(len(r) == L for r in wb["rows"]) and all(len(p) == 3 * L + 64 for p in wb["proofs"])
    return PedersenSharedWireBatch(wb["n"], b"".join(wb["rows"]), wb["input_index"], b"".join(wb["outputs"]), wb["io_counts"],
                                   b"".join(wb["ads"]), [len(a) for a in wb["ads"]], b"".join(wb["proofs"]), L)
