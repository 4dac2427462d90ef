"""GPU: state carried from one run of a staged batch to the next on ONE context (include/avrf.h: avrf_*_batch_run, the three-call run,
avrf_*_batch_run_segments / _shared_segments, the as-MSM route of avrf_*_verify, avrf_*_batch_challenges, open batches).

Every entry point that runs a staged batch goes through one run record and one set of phases (capi_internal.h run_begin .. run_end), so
what one run leaves behind -- the phase, the shape of the last segmented run, the weight choice, the term arrays -- is what the next one
finds.  A sequence of runs of every kind is walked on one context, and after EVERY step
  * the verdict or the statuses are the CPU oracle's on that step's items,
  * avrf_batch_last_terms, or every segment's avrf_*_segment_terms, equal byte for byte what a FRESH context gives that performs only
    that step (and the oracle's terms, where the oracle states them in the device's layout),
  * the context is idle (avrf_ctx_busy_).
40 items with 0 to 3 pairs, Thin and Pedersen, a counter-mode suite (0) and a sponge suite (5); the segment lists sit on both sides of the
eight-segment threshold between the looped and the chained MSM route; the shared-table stagings (one pair per item, 4 rows) take the
merged layout for both lists.  The oracle's results are computed once per module and shared."""
import ctypes as C
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import oracle as orc
from helpers import R_ORDER, nat_batch, xy

import ped_shared_helpers as ph
import shared_segments_helpers as sh
import test_gpu_pedersen_segments as ped
import test_gpu_thin_segments as thin

pytestmark = pytest.mark.gpu

THIN, PEDERSEN = 1, 2
SUITES = [0, 5]
N, BAD, ONE = 40, 27, 3
SEGS2 = [20, 20]                          # fewer than eight segments: one MSM each, looped
SEGS9 = [1, 2, 3, 4, 5, 6, 7, 8, 4]       # nine: one chain
CHUNKS = [(0, 13), (13, 27), (27, 40)]
COUNTS = random.Random(11).choices(range(4), k=N)       # pairs per item, 0 to 3
T_ROWS = 4


def busy(c):
    from ark_vrf_amd import _native as nat
    return nat.lib().avrf_ctx_busy_(c._h)


def segment_of(segs, j):
    at = 0
    for v, k in enumerate(segs):
        at += k
        if j < at:
            return v
    raise AssertionError(j)


# ---------------------------------------------------------------- material: what a sequence runs on, with the oracle's answers cached

class Plain:
    """40 plain items of one kind; variant: None, "flip" (item 27's s with a bit flipped: the equation fails) or "range" (s = r: refused)"""
    _made, _oracle = {}, {}

    def __init__(self, suite, kind, variant=None):
        self.suite, self.kind, self.mod, self.key = suite, kind, thin if kind == THIN else ped, (suite, kind, variant)
        if (suite, kind) not in Plain._made:
            Plain._made[suite, kind] = self.mod.made_items(suite, COUNTS, 50 + kind)
        self.items = list(Plain._made[suite, kind])
        at = 64 if kind == THIN else 192                                               # where s is in the x || y proof
        it = self.items[BAD]
        if variant == "flip":
            self.items[BAD] = thin.tamper_s(it) if kind == THIN else ped.tamper(it, 0)
        elif variant == "range":
            self.items[BAD] = dict(it, proof=it["proof"][:at] + R_ORDER[suite].to_bytes(32, "little") + it["proof"][at + 32:])

    def batch(self, lo=0, hi=N):
        return nat_batch(self.mod.batch_dict(self.items[lo:hi]))

    def oracle(self, lo=0, hi=N):
        """(status, bases, scalars) of items [lo, hi) as a batch of their own"""
        k = self.key + (lo, hi)
        if k not in Plain._oracle:
            Plain._oracle[k] = self.mod.oracle_segment(self.suite, self.items[lo:hi])
        return Plain._oracle[k]

    def oracle_segments(self, segs):
        out, at = [], 0
        for k in segs:
            out.append(self.oracle(at, at + k)); at += k
        return out

    def stage(self, c):
        return c.thin_batch_stage(self.batch()) if self.kind == THIN else c.pedersen_batch_stage(self.batch())

    def run(self, c):
        return c.thin_batch_run() if self.kind == THIN else c.pedersen_batch_run()

    def run_segments(self, c, segs):
        return c.thin_batch_run_segments(segs) if self.kind == THIN else c.pedersen_batch_run_segments(segs)

    def segment_terms(self, c, v):
        return c.thin_segment_terms(v) if self.kind == THIN else c.pedersen_segment_terms(v)

    def verify_one(self, c, j):
        return c.thin_verify(self.batch(j, j + 1)) if self.kind == THIN else c.pedersen_verify(self.batch(j, j + 1))

    def challenges(self, c):
        from ark_vrf_amd import _native as nat
        out = (C.c_uint8 * (16 * N))()
        f = nat.lib().avrf_thin_batch_challenges if self.kind == THIN else nat.lib().avrf_pedersen_batch_challenges
        return f(c._h, out), bytes(out)

    def open_and_push(self, c):
        assert c.batch_open(self.kind) == 0
        for lo, hi in CHUNKS:
            assert c.batch_push(self.kind, self.batch(lo, hi)) == 0
        assert c.batch_pushed()[0] == N
        return 0


def thin_shared40(suite):
    """a VERIFYING Thin batch of 40 one-pair items over 4 rows made of the items' own keys (rows 0, 1) and inputs (rows 2, 3): item j has
    key j % 2 and input 2 + (j // 2) % 2; proofs by the oracle's prover"""
    L = orc.pt_len(suite)
    keys = [orc.from_seed(suite, bytes([k + 1, 61]) + bytes(30)) for k in range(2)]
    rows_c = [pk for _, pk in keys] + [orc.hash_to_curve(suite, b"seq-slot-%d" % i) for i in range(2)]
    outs = {(k, r): orc.vrf_output(suite, keys[k][0], rows_c[r]) for k in range(2) for r in (2, 3)}
    plan = [(j % 2, 2 + (j // 2) % 2, b"ad-%d" % j * (j % 3)) for j in range(N)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        proofs = list(ex.map(lambda p: orc.thin_prove(suite, keys[p[0]][0], [(rows_c[p[1]], outs[p[0], p[1]])], p[2]), plan))
    return dict(n=N, rows=[xy(suite, r) for r in rows_c], pk_index=[k for k, _, _ in plan], input_index=[r for _, r, _ in plan],
                outputs=[xy(suite, outs[k, r]) for k, r, _ in plan], io_counts=[1] * N, ads=[ad for _, _, ad in plan],
                proofs=[xy(suite, p[:L]) + p[L:] for p in proofs])


class Shared:
    """the 40 items with one pair each over a table of 4 rows"""
    _made = {}

    def __init__(self, suite, kind):
        self.suite, self.kind, self.key = suite, kind, ("seq40", suite, kind)
        if (suite, kind) not in Shared._made:
            Shared._made[suite, kind] = thin_shared40(suite) if kind == THIN else ph.real_batch(suite, [1] * N, T_ROWS, seed=62)
        self.sb = Shared._made[suite, kind]
        assert len(self.sb["rows"]) == T_ROWS

    def oracle(self):
        return sh.oracle_of(self.suite, self.key, self.sb, [N])[0]

    def oracle_segments(self, segs):
        return sh.oracle_of(self.suite, self.key, self.sb, segs)

    def stage(self, c):
        return sh.stage(c, self.sb)

    def run(self, c):
        return c.thin_batch_run() if self.kind == THIN else c.pedersen_batch_run()

    def run_segments(self, c, segs):
        return sh.run(c, self.sb, segs)

    def segment_terms(self, c, v):
        return sh.segment_terms(c, self.sb, v)


# ---------------------------------------------------------------- steps: act(c, M) -> (result, terms)

def step_stage(c, M):
    return M.stage(c), None


def step_plain(c, M):
    return M.run(c), c.last_terms()


def step_three(c, M):
    assert c.batch_run_begin() == 0 and busy(c)
    st = c.batch_run_hash()                                                            # (a refused item shows here, and closes the run)
    if st != 0:
        return st, c.last_terms()
    assert busy(c)
    return c.batch_run_end(), c.last_terms()


def step_segments(segs):
    def act(c, M):
        got = M.run_segments(c, segs)
        assert isinstance(got, list), got
        return got, [M.segment_terms(c, v) for v in range(len(segs))]
    return act


def step_one(c, M):
    return M.verify_one(c, ONE), c.last_terms()


def step_challenges(c, M):
    return M.challenges(c)


def step_open(c, M):
    return M.open_and_push(c), None


def step_open_run(c, M):
    M.open_and_push(c)
    return step_plain(c, M)


# name -> (what a fresh context does first, the step)
STEPS = {"stage": (None, step_stage), "plain": (step_stage, step_plain), "three": (step_stage, step_three),
         "segs2": (step_stage, step_segments(SEGS2)), "segs9": (step_stage, step_segments(SEGS9)), "one": (None, step_one),
         "challenges": (step_stage, step_challenges), "open_run": (None, step_open_run), "open_segs9": (step_open, step_segments(SEGS9))}
SEQUENCE = ["stage", "plain", "segs2", "three", "segs9", "plain", "one", "stage", "challenges", "plain", "open_run", "open_segs9"]
_FRESH = {}


def fresh(M, name):
    """what a fresh context gives that performs only this step (behind the staging the step needs)"""
    from ark_vrf_amd import _native as nat
    if (M.key, name) not in _FRESH:
        c = nat.Context(M.suite)
        try:
            first, act = STEPS[name]
            if first:
                assert first(c, M)[0] == 0
            _FRESH[M.key, name] = act(c, M)
            assert not busy(c)
        finally:
            c.close()
    return _FRESH[M.key, name]


def expected(M, name):
    """the oracle's (result, terms) of a step; terms None where the oracle does not state them in the device's layout"""
    plain_layout = isinstance(M, Plain)
    if name in ("stage",):
        return 0, None
    if name in ("plain", "three", "open_run"):
        st, bases, sc = M.oracle()
        return st, (bases, sc) if plain_layout and st != 2 else None
    if name in ("segs2", "segs9", "open_segs9"):
        want = M.oracle_segments(SEGS2 if name == "segs2" else SEGS9)
        return [w[0] for w in want], [(w[1], w[2]) if w[0] != 2 else None for w in want] if plain_layout else None
    if name == "one":
        return [M.oracle(ONE, ONE + 1)[0]], None
    assert name == "challenges"
    return 0, None


def walk(c, M, names):
    for at, name in enumerate(names):
        got, terms = STEPS[name][1](c, M)
        where = (M.key, at, name)
        assert not busy(c), where
        want, want_terms = expected(M, name)
        assert got == want, (where, got, want)
        f_got, f_terms = fresh(M, name)
        assert got == f_got, where
        # (a refused batch or segment: the oracle builds no terms, and what the device holds for it is not defined)
        if isinstance(got, list) and isinstance(terms, list):
            assert [t for t, st in zip(terms, got) if st != 2] == [t for t, st in zip(f_terms, got) if st != 2], where
        elif got != 2:
            assert terms == f_terms, where
        if isinstance(want_terms, list):
            for v, w in enumerate(want_terms):
                if w is not None:
                    assert terms[v] == w, (where, v)
        elif want_terms is not None:
            assert terms == want_terms, where


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


# ---------------------------------------------------------------- the tests

@pytest.mark.parametrize("suite", SUITES)
@pytest.mark.parametrize("kind", [THIN, PEDERSEN])
def test_every_run_in_turn(ctxs, suite, kind):
    """stage, plain, two segments, three calls, nine segments, plain, one item through avrf_*_verify (which restages), stage, challenges,
    plain, an open batch pushed as three chunks and run, nine segments on the open batch -- all on one context"""
    M = Plain(suite, kind)
    assert M.oracle()[0] == 0
    walk(ctxs[suite], M, SEQUENCE)


@pytest.mark.parametrize("suite", SUITES)
@pytest.mark.parametrize("kind", [THIN, PEDERSEN])
@pytest.mark.parametrize("variant", ["flip", "range"])
def test_one_bad_item(ctxs, suite, kind, variant):
    """item 27 bad -- its equation fails (flip), or its response is refused, which sends the segmented runs through the per-item
    attribution pass (range): the plain verdicts are the oracle's, exactly the segment holding item 27 carries the oracle's status for
    it, and the context is idle after every step"""
    M = Plain(suite, kind, variant)
    st_bad = {"flip": 1, "range": 2}[variant]
    assert M.oracle()[0] == st_bad
    for segs in (SEGS2, SEGS9):
        v = segment_of(segs, BAD)
        assert [w[0] for w in M.oracle_segments(segs)] == [st_bad if u == v else 0 for u in range(len(segs))]
    walk(ctxs[suite], M, SEQUENCE[:6])


@pytest.mark.parametrize("suite", SUITES)
@pytest.mark.parametrize("kind", [THIN, PEDERSEN])
def test_shared_table_runs_in_turn(ctxs, suite, kind):
    """the same 40 items with one pair each over a table of 4 rows: both segment lists take the merged layout (Thin 20 + 20 + 4 + 1 = 45
    terms against 2 * 20 + 2 * 20 + 1 = 81, Pedersen 4 * 20 + 4 + 2 = 86 against 5 * 20 + 2 = 102), and stage, plain, two segments,
    three calls, nine segments, plain run on one context"""
    from ark_vrf_amd import _native as nat
    M = Shared(suite, kind)
    for segs, want_L in ((SEGS2, 45 if kind == THIN else 86), (SEGS9, 21 if kind == THIN else 38)):
        lay = nat.thin_shared_segments_layout(segs, [1] * N, T_ROWS) if kind == THIN else nat.pedersen_shared_segments_layout(N, segs, T_ROWS)
        assert lay == sh.py_layout(kind == THIN, segs, [1] * N, T_ROWS) and lay[4] == 1 and lay[0] == want_L, lay
    assert M.oracle()[0] == 0
    walk(ctxs[suite], M, SEQUENCE[:6])
