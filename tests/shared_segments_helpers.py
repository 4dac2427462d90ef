"""Helpers of the segmented shared-table tests (include/avrf.h avrf_thin_batch_run_shared_segments,
avrf_pedersen_batch_run_shared_segments): the layout arithmetic in Python, a shared batch cut into its segments, and the oracle's terms of
ONE SEGMENT'S EXPANDED ITEMS folded into that segment's merged layout.

A shared batch is a dict as in ped_shared_helpers (rows, input_index, outputs, io_counts, ads, proofs; n), a Thin one with pk_index as
well.  A segment's merged layout IS the shared layout of a batch of just its items over the same table, so the folding is the whole-batch
folding applied to the segment's sub-batch: ped_shared_helpers.check_terms for Pedersen, fold_thin below for Thin."""
import oracle as orc
from helpers import R_ORDER

import ped_shared_helpers as ph


def is_thin(sb):
    return "pk_index" in sb


def window_bits(L):
    """what the engine's plan gives an L-term MSM below 65 536 terms: floor(log2 L) - 3, at least 4"""
    return max(4, L.bit_length() - 1 - 3)


def py_layout(thin, seg_items, io_counts, T):
    """-> (L, n_seg L, sum of n_v, window bits, mode): the arithmetic of include/avrf.h "layouts" restated.  io_counts: per item (Thin)."""
    at, plain, merged = 0, [], []
    for k in seg_items:
        p = sum(io_counts[at: at + k]) if thin else 0
        plain.append((2 * k + 2 * p + 1 if thin else 5 * k + 2) if k else 0)
        merged.append(((k + p + T + 1) if thin else 4 * k + T + 2) if k else 0)
        at += k
    L_p, L_m = max(plain, default=0), max(merged, default=0)
    mode = 1 if T and L_m < L_p else 0
    L, counts = (L_m, merged) if mode else (L_p, plain)
    return (L, len(seg_items) * L, sum(counts), window_bits(L) if L else 0, mode)


def sub_batches(sb, segs):
    """the shared batch of every segment's items alone, over the same table"""
    out, at, io = [], 0, 0
    for k in segs:
        m = sum(sb["io_counts"][at: at + k])
        sub = dict(sb, n=k, input_index=sb["input_index"][io: io + m], outputs=sb["outputs"][io: io + m], io_counts=sb["io_counts"][at: at + k],
                   ads=sb["ads"][at: at + k], proofs=sb["proofs"][at: at + k])
        if is_thin(sb):
            sub["pk_index"] = sb["pk_index"][at: at + k]
        out.append(sub); at += k; io += m
    assert at == sb["n"]
    return out


def expanded(sb):
    """the plain batch a shared one stands for (a gen_batch-style dict)"""
    e = ph.expanded(sb)
    if is_thin(sb):
        e["pks_xy"] = b"".join(sb["rows"][r] for r in sb["pk_index"])
    return e


def oracle_segment(suite, sub):
    """(status, bases, scalars) of the oracle on the segment's EXPANDED items alone; an empty segment is Ok and has no terms"""
    if not sub["n"]:
        return 0, b"", b""
    e = expanded(sub)
    if is_thin(sub):
        st, bases, sc = orc.thin_batch_terms_xy(suite, e)
        return (orc.thin_batch_verify_xy(suite, e) if st == 0 else st), bases, sc
    st, bases, sc = orc.pedersen_batch_terms_xy(suite, e)
    return (orc.pedersen_batch_verify_xy(suite, e) if st == 0 else st), bases, sc


def fold_thin(suite, sub, bases, sc):
    """oracle terms (R, pk, (O_i, I_i).., G) of a segment's expanded items -> (bases, scalars) in its merged layout: (R_j, w_j) at
    j + io0 with its outputs behind it, row r at n + tot + r with the key and input scalars added mod r_order, (G, g) last"""
    n, tot, rows, r_order = sub["n"], sum(sub["io_counts"]), sub["rows"], R_ORDER[suite]
    assert len(sc) == 32 * (2 * n + 2 * tot + 1)
    term = lambda k: (bases[64 * k: 64 * k + 64], sc[32 * k: 32 * k + 32])
    out, acc = [None] * (n + tot + len(rows) + 1), [0] * len(rows)
    k = io0 = 0
    for j, m in enumerate(sub["io_counts"]):
        out[j + io0] = term(k)
        pb, ps = term(k + 1)
        assert pb == rows[sub["pk_index"][j]]
        acc[sub["pk_index"][j]] += int.from_bytes(ps, "little")
        for i in range(m):
            out[j + io0 + 1 + i] = term(k + 2 + 2 * i)
            ib, is_ = term(k + 3 + 2 * i)
            assert ib == rows[sub["input_index"][io0 + i]]
            acc[sub["input_index"][io0 + i]] += int.from_bytes(is_, "little")
        k += 2 + 2 * m; io0 += m
    for r, row in enumerate(rows):
        out[n + tot + r] = (row, (acc[r] % r_order).to_bytes(32, "little"))
    out[-1] = term(k)
    return b"".join(t[0] for t in out), b"".join(t[1] for t in out)


def nat_shared(sb):
    if not is_thin(sb):
        return ph.nat_shared(sb)
    from ark_vrf_amd._native import SharedBatch
    return SharedBatch(sb["n"], b"".join(sb["rows"]), sb["pk_index"], sb["input_index"], b"".join(sb["outputs"]), sb["io_counts"],
                       b"".join(sb["ads"]), [len(a) for a in sb["ads"]], b"".join(sb["proofs"]))


def stage(c, sb):
    return c.thin_batch_stage_shared(nat_shared(sb)) if is_thin(sb) else c.pedersen_batch_stage_shared(nat_shared(sb))


def run(c, sb, segs):
    return c.thin_batch_run_shared_segments(segs) if is_thin(sb) else c.pedersen_batch_run_shared_segments(segs)


def segment_terms(c, sb, v):
    return c.thin_segment_terms(v) if is_thin(sb) else c.pedersen_segment_terms(v)


_THIN = {}


def thin_real_batch(suite, counts, seed=1):
    """a VERIFYING Thin batch of len(counts) items with counts[j] pairs each over T = 5 rows: keys 0..2, hashed inputs 3 and 4 -- and row 0,
    key 0's point, is an input as well, so that a row is referenced both ways.  Item j has key j % 3; proofs by the oracle's prover."""
    import random
    from concurrent.futures import ThreadPoolExecutor
    from helpers import xy
    key = (suite, tuple(counts), seed)
    if key in _THIN:
        return _THIN[key]
    rng = random.Random(seed)
    L = orc.pt_len(suite)
    keys = [orc.from_seed(suite, bytes([k + 1, seed]) + bytes(30)) for k in range(3)]
    rows_c = [pk for _, pk in keys] + [orc.hash_to_curve(suite, b"slot-%d" % i) for i in range(2)]
    outs = {(k, r): orc.vrf_output(suite, keys[k][0], rows_c[r]) for k in range(3) for r in (0, 3, 4)}
    items = [(j % 3, [rng.choice((0, 3, 4)) for _ in range(m)], b"ad-%d" % j * (j % 3)) for j, m in enumerate(counts)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        proofs = list(ex.map(lambda it: orc.thin_prove(suite, keys[it[0]][0], [(rows_c[r], outs[it[0], r]) for r in it[1]], it[2]), items))
    out_xy = {kr: xy(suite, o) for kr, o in outs.items()}
    sb = dict(n=len(counts), rows=[xy(suite, r) for r in rows_c], pk_index=[k for k, _, _ in items], input_index=[r for _, rr, _ in items for r in rr],
              outputs=[out_xy[k, r] for k, rr, _ in items for r in rr], io_counts=list(counts), ads=[ad for _, _, ad in items],
              proofs=[xy(suite, p[:L]) + p[L:] for p in proofs])
    _THIN[key] = sb
    return sb


def with_rows(sb, rows):
    return dict(sb, rows=list(rows))


def segments_referencing(sb, segs, r):
    """the segments with an item whose key or one of whose inputs is row r"""
    return [v for v, sub in enumerate(sub_batches(sb, segs)) if r in sub["input_index"] or r in sub.get("pk_index", [])]


_ORACLE = {}


def oracle_of(suite, key, sb, segs):
    """the oracle's (status, bases, scalars) per segment, computed once per (key, segs) and shared"""
    k = (suite, is_thin(sb), key, tuple(segs))
    if k not in _ORACLE:
        _ORACLE[k] = [oracle_segment(suite, sub) for sub in sub_batches(sb, segs)]
    return _ORACLE[k]


def check_segments(c, suite, sb, segs, want_mode, key=None, staged=False):
    """stage (unless staged), run the segments through the new call, compare every status with the oracle on the segment's expanded items
    alone and every segment's terms with the oracle's in the layout the run must have chosen (want_mode); -> statuses"""
    from ark_vrf_amd import _native as nat
    thin, T = is_thin(sb), len(sb["rows"])
    lay = py_layout(thin, segs, sb["io_counts"], T)
    assert lay[4] == want_mode, lay
    assert (nat.thin_shared_segments_layout(segs, sb["io_counts"], T) if thin else nat.pedersen_shared_segments_layout(sb["n"], segs, T)) == lay
    if not staged:
        assert stage(c, sb) == 0
    got = run(c, sb, segs)
    assert isinstance(got, list) and len(got) == len(segs), got
    subs = sub_batches(sb, segs)
    want = oracle_of(suite, key, sb, segs) if key is not None else [oracle_segment(suite, sub) for sub in subs]
    for v, (sub, (st, bases, sc)) in enumerate(zip(subs, want)):
        assert got[v] == st, (v, got, st)
        gb, gs = segment_terms(c, sb, v)
        if not sub["n"]:
            assert gb == b"" and gs == b""
        elif st == 2:
            continue                                                               # (the oracle builds no terms for a refused batch)
        elif not want_mode:
            assert gs == sc and gb == bases, v
        elif thin:
            wb, ws = fold_thin(suite, sub, bases, sc)
            assert gs == ws and gb == wb, v
        else:
            ph.check_terms(suite, sub, (gb, gs))
    return got
