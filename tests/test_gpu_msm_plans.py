"""GPU parity of the Pippenger chain (csrc/msm.hip) under EVERY plan, not only the ones msm_plan picks for the sizes other tests use:
window widths c = 4 .. 15, entries per lane 1 .. 4 096, the window-sum and the bit-sum tail, other occupancies, the general chain at
tiny sizes -- each on inputs built for it (tests/msm_plan_inputs.py, conditions checked by tests/test_msm_plan_inputs_host.py),
through five chains: avrf_msm_te on Bandersnatch, Baby-JubJub and secp256r1 (the native short-Weierstrass suite), avrf_g1_msm on
BLS12-381 and BN254 -- and, beside them, avrf_msm_te_segments on Bandersnatch (the batched tail: k_bits_direct or k_rowcol / k_bits,
the device Horner) and the ring commitment of both pairing suites down the general chain (three G1 vectors in one call).

The engine reads its knobs once per process, so a case is one fresh child (tests/msm_plan_child.py) with the knobs in its
environment; the child reports every result and the plan avrf_kernel_stats gives after it.  A result must equal the reference byte
for byte, and the plan must be the one asked for: a knob that is silently ignored fails.

References, computed once: orc.msm (oracle/orc_msm.c, Pippenger) -- for `mix` held against the naive double-and-add (algo 0) and
against the collapsed sum (scalars added per distinct base in Python integers) -- and oracle/ring_py.py's big-int MSM for G1.

After a child that timed out or died by a signal nothing more is started: the remaining cases fail at once."""
import json
import os
import random
import subprocess
import sys
import time

import pytest

import msm_plan_inputs as mpi
import oracle as orc
from oracle import ring_py as R
from helpers import IDENTITY_XY, R_ORDER, rand_points_xy, xy

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "msm_plan_child.py")
SRS = {0: "bls12-381-srs-2-11-uncompressed-zcash.bin", 1: "bn254-testing-2-9-uncompressed.bin"}
RING_VECTORS = {0: "bandersnatch_sha-512_ell2_ring.json", 1: "baby-jubjub_sha-512_tai_ring.json"}
FIELD = {0: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
         1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
         7: 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff}
SEED = 4100
SEG_N, SEG_L = 8, 350
_stopped = []                              # why nothing more may be started on the GPU (the stopping rule)


# ---------------------------------------------------------------- terms -> the bytes of one chain, and its reference

class TeChain:
    """avrf_msm_te on a suite: x || y of 32 bytes each; -(x, y) = (-x, y) on a twisted Edwards curve, (x, -y) on secp256r1, whose
    identity is 64 zero bytes in this ABI"""
    call = "msm"

    def __init__(self, suite):
        self.suite, self.r = suite, R_ORDER[suite]
        self.points = rand_points_xy(random.Random(SEED + suite), suite, mpi.TILES3_BASES)
        self.identity = bytes(64) if suite == orc.SECP256R1 else IDENTITY_XY

    def base(self, i, neg):
        if i < 0:
            return self.identity
        p, q = self.points[i], FIELD[self.suite]
        x, y = int.from_bytes(p[:32], "little"), int.from_bytes(p[32:], "little")
        if neg and self.suite == orc.SECP256R1:
            y = (q - y) % q
        elif neg:
            x = (q - x) % q
        return x.to_bytes(32, "little") + y.to_bytes(32, "little")

    def reference(self, bases, ks, algo=1):
        return orc.msm(self.suite, b"".join(bases), b"".join(k.to_bytes(32, "little") for k in ks), algo) if ks else self.identity


class G1Chain:
    """avrf_g1_msm of Context(i): little-endian x || y of the pairing curve's base field, (0, 0) the point at infinity; bases from the
    reference's SRS files"""
    call = "g1_msm"

    def __init__(self, i, golden_dir):
        self.suite, self.s = i, R.SUITES[i]
        self.r = self.s.r
        self.points = R.Srs(self.s, open(os.path.join(golden_dir, SRS[i]), "rb").read()).g1[:mpi.TILES3_BASES]

    def base(self, i, neg):
        n = self.s.fp_bytes
        if i < 0:
            return bytes(2 * n)
        x, y = self.points[i]
        return x.to_bytes(n, "little") + ((-y) % self.s.p if neg else y).to_bytes(n, "little")

    def reference(self, bases, ks, algo=1):
        n = self.s.fp_bytes
        pts = [None if b == bytes(2 * n) else (int.from_bytes(b[:n], "little"), int.from_bytes(b[n:], "little")) for b in bases]
        P = R.g1_affine(self.s.p, R.g1_msm(self.s.p, pts, ks))
        return bytes(2 * n) if P is None else P[0].to_bytes(n, "little") + P[1].to_bytes(n, "little")


def make_set(chain, terms, check_naive=False):
    """-> (the child's input set, the expected result)"""
    bases, ks = [chain.base(i, neg) for i, neg, _ in terms], [k for _, _, k in terms]
    want = chain.reference(bases, ks)
    if len(set(bases)) < len(bases):                     # repeated bases: the same sum with every distinct base once
        assert chain.reference(*mpi.collapse(bases, ks, chain.r)) == want
    if check_naive:                                      # double-and-add: the reference is not one Pippenger checking another
        assert chain.reference(bases, ks, algo=0) == want
    return dict(call=chain.call, suite=chain.suite, bases=b"".join(bases).hex(), scalars=b"".join(k.to_bytes(32, "little") for k in ks).hex()), want


@pytest.fixture(scope="module")
def world(golden_dir, tmp_path_factory):
    """-> ({kind of case: its case file, written once}, {kind: {set: expected bytes}}, {kind: {set: (terms per MSM, MSMs, bits of the
    group order, the scalars)}})"""
    chains = {"te0": TeChain(0), "te1": TeChain(1), "te7": TeChain(7), "g1_0": G1Chain(0, golden_dir), "g1_1": G1Chain(1, golden_dir)}
    sets, want, shape = ({"mix": {}, "small": {}, "tiles3": {}, "ring": {}} for _ in range(3))

    def put(kind, name, ch, terms, n_seg=1, **kw):
        L = len(terms) // n_seg
        parts = [make_set(ch, terms[v * L: (v + 1) * L], **kw) for v in range(n_seg)]
        sets[kind][name] = dict(parts[0][0], bases="".join(p[0]["bases"] for p in parts), scalars="".join(p[0]["scalars"] for p in parts))
        want[kind][name] = b"".join(p[1] for p in parts)
        shape[kind][name] = (L, n_seg, ch.r.bit_length(), [k for _, _, k in terms])

    for name, ch in chains.items():
        put("mix", name, ch, mpi.mix_terms(ch.r, SEED)[0], check_naive=isinstance(ch, TeChain))
        for n, terms in mpi.small_terms(ch.r, SEED).items():
            put("small", "%s_%d" % (name, n), ch, terms)
    for name in ("te0", "te7"):
        put("tiles3", name, chains[name], mpi.tiles3_terms(chains[name].r, SEED))
    # the segmented call on the first SEG_N x SEG_L terms of Bandersnatch's mix: every segment against the oracle on its terms alone
    put("mix", "te0_segments", chains["te0"], mpi.mix_terms(chains["te0"].r, SEED)[0][:SEG_N * SEG_L], n_seg=SEG_N)
    sets["mix"]["te0_segments"].update(call="msm_segments", n_seg=SEG_N)
    # the ring commitment of the first reference ring vector of each pairing suite: three KZG commits of 512 terms in one G1 call
    for i, vec in RING_VECTORS.items():
        with open(os.path.join(golden_dir, vec)) as f:
            v = json.load(f)[0]
        raw = bytes.fromhex(v["ring_pks"])
        keys = b"".join(xy(i, raw[k: k + 32]) for k in range(0, len(raw), 32))
        sets["ring"]["g1_%d" % i] = dict(call="ring_commit", suite=i, srs=os.path.join(golden_dir, SRS[i]), keys=keys.hex())
        want["ring"]["g1_%d" % i] = bytes.fromhex(v["ring_pks_com"])
    d = tmp_path_factory.mktemp("msm_plans")
    files = {}
    for kind, v in sets.items():
        files[kind] = str(d / (kind + ".json"))
        with open(files[kind], "w") as f:
            json.dump(v, f)
    return files, want, shape


# ---------------------------------------------------------------- one case = one child

def run_case(world, which, knobs):
    """start the child on case file `which` with `knobs` added to this process's environment -> (its report, the expected bytes, the
    shape of every set)"""
    files, want, shape = world
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    env = dict(os.environ)
    env.update(knobs)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, CHILD, files[which]], env=env, timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        _stopped.append("the child of %s %r timed out\nstdout: %s\nstderr: %s" % (which, knobs, e.stdout, e.stderr))
        pytest.fail(_stopped[0])
    if p.returncode < 0 or p.returncode in (134, 137, 139):
        _stopped.append("the child of %s %r died with status %d\nstdout: %s\nstderr: %s" % (which, knobs, p.returncode, p.stdout, p.stderr))
        pytest.fail(_stopped[0])
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print("\ncase %s %s: %.1f s" % (which, " ".join("%s=%s" % kv for kv in sorted(knobs.items())) or "(default)", time.perf_counter() - t0))
    for name in sorted(got):
        print("  %-14s plan %s" % (name, got[name].get("plan", got[name])))
    assert sorted(got) == sorted(want[which])
    return got, want[which], shape[which]


def default_width(n):
    """msm_plan's choice for n terms (restated: the cases that leave the width alone still say which width ran)"""
    lg = n.bit_length() - 1
    return min(15, max(4, lg - 5 if lg >= 16 else lg - 3))


def shares(per_min, c, n_seg, bits, ks):
    """the entries per lane k_plan may report for these scalars: per_min, unless the chain's entries (the non-zero digits) exceed one
    residency round of its k_accumulate -- a whole number of 256-lane workgroups on each of the MI355X's 256 CUs, less a lane per
    window -- and then ceil(entries / round).  Every chain but secp256r1's holds `mix` in one round at every width (so the only value
    is per_min); that kernel holds 65 536 lanes, and 33 windows of `mix` at c = 8 are some 80 000 entries: 2 per lane.  A knob that was
    not read leaves 8 and fails either way."""
    vwin = n_seg * mpi.nwin(bits, c)
    entries = sum(1 for k in ks for b, _ in mpi.recode(k, c, mpi.nwin(bits, c)) if b)
    return {max(per_min, -(-entries // (65536 * blocks - vwin))) for blocks in range(1, 9)}


def check(world, which, knobs, c=None, per=None):
    """every result equals its reference, and every chain ran the plan asked for: width `c` (None: msm_plan's own), `per` entries per lane"""
    got, want, shape = run_case(world, which, knobs)
    for name, g in got.items():
        n, n_seg, bits, ks = shape[name]
        assert "error" not in g, (name, g)
        assert bytes.fromhex(g["out"]) == want[name], name
        wc = c if c is not None else default_width(n)
        assert g["plan"][:3] == [wc, mpi.nwin(bits, wc), 1 << (wc - 1)], (name, g["plan"], wc)
        assert g["plan"][3] >= 1                                   # (the single launch reports 0: the chain ran)
        if per is not None:
            assert g["plan"][3] in shares(per, wc, n_seg, bits, ks), (name, g["plan"], per)


@pytest.mark.parametrize("c", list(mpi.WIDTHS))
def test_window_width(world, c):
    check(world, "mix", {"AVRF_MSM_C": str(c)}, c=c)


@pytest.mark.parametrize("c", [8, 13])
@pytest.mark.parametrize("per", [1, 3, 64, 4096])
def test_lane_share(world, c, per):
    """per = 1: every lane holds one entry and k_bucket_sum / k_heavy_sum do all the additions; 3 divides no bucket; 64: the 800-entry
    bucket is heavy, the others are walked by one or two lanes; 4 096: one lane walks a whole window, runs of empty buckets included.
    (The totals are below one residency round of the kernels, so per_min decides -- but for secp256r1 at per_min = 1: see `shares`.)"""
    check(world, "mix", {"AVRF_MSM_C": str(c), "AVRF_MSM_PER_MIN": str(per)}, c=c, per=per)


@pytest.mark.parametrize("c,per", [(4, None), (8, None), (9, None), (10, None), (13, None), (15, None), (9, 1)])
def test_bit_sum_tail(world, c, per):
    """AVRF_TE_WINDOW_SUMS=0 puts the twisted-Edwards suites on k_rowcol / k_bits, where G1 and secp256r1 always are: h = (c - 1) / 2
    of both parities, nb below and above a wave per row"""
    knobs = {"AVRF_MSM_C": str(c), "AVRF_TE_WINDOW_SUMS": "0"}
    if per:
        knobs["AVRF_MSM_PER_MIN"] = str(per)
    check(world, "mix", knobs, c=c, per=per)


@pytest.mark.parametrize("occ", [1, 3])
def test_occupancy(world, occ):
    """AVRF_MSM_OCC: the LDS-slice cap of accumulate_shape and another lanes_target, at msm_plan's own width"""
    check(world, "mix", {"AVRF_MSM_OCC": str(occ)})


def test_general_chain_at_tiny_sizes(world):
    """AVRF_MSM_TINY=0: 1, 2, 5, 64 and 300 terms down the general chain -- lanes with empty shares, windows without entries, c = 4"""
    check(world, "small", {"AVRF_MSM_TINY": "0"})


def test_g1_three_vectors_general_chain(world):
    """AVRF_MSM_TINY=0 sends the ring commitment's G1 call -- 3 scalar vectors over 512 SRS points, inside the single launch by default --
    down the general chain (c = 6): bit sums of every vector come back and their Horners run side by side on the host.  The
    commitment must be the reference vector's"""
    got, want, _ = run_case(world, "ring", {"AVRF_MSM_TINY": "0"})
    for name, g in got.items():
        assert "error" not in g, (name, g)
        assert bytes.fromhex(g["out"]) == want[name], name


def test_three_tiles_default_environment(world):
    """16 391 terms: three sort tiles, the last one of seven keys, under whatever plan the defaults give"""
    check(world, "tiles3", {})


def test_width_below_range_is_ignored(world):
    """AVRF_MSM_C=3 is outside the knob's range (4 .. 15): msm_plan's own width runs, and the result is right"""
    check(world, "mix", {"AVRF_MSM_C": "3"})
