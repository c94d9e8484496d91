"""Case table of the step-API tests, shared by tests/test_gpu_step_api.py (one launch per case on the device) and
tests/test_step_cases.py (the same table checked without a GPU: its coverage, and that it tells the mutants of the mirror apart).

A case names an entry point, the dtype, chunk_rows, n_local, g_red, `it`, maxiter, the state of the scalar block before the call
and the `kinds` that make it special.  inputs(case) builds its operands deterministically (seeded by the case id); expected(case,
inp, mirror) runs tests/_step_mirror.py on copies and returns every output: the vectors, all 2048 slots of every partial array and
the first 8 words of the scalar block."""
import types
import zlib

import numpy as np

import _step_mirror as sm
from oracle import oracle as O

# argument lists of the entry points in the order of include/hipk.h: "@name" a vector operand, "#name" a partial array
ARGS = {
    "cg_start": ("n", "ch", "g", "scal", "#part_rr", "#part_bb", "@r", "@p", "dt", "tol", "atol", "maxiter", "stream"),
    "cg_update": ("n", "ch", "g", "scal", "it", "#part_pAp", "@Ap", "@r", "#part_out", "dt", "stream"),
    "cg_direction": ("n", "ch", "g", "scal", "it", "maxiter", "#part_pAp", "#part_rr", "@r", "@p", "@x", "dt", "stream"),
    "cg_xupdate": ("n", "ch", "g", "scal", "it", "#part_pAp", "@p", "@x", "dt", "stream"),
    "cgm_start": ("n", "ch", "g", "scal", "#part_rz", "#part_rr", "#part_bb", "@z", "@p", "dt", "tol", "atol", "maxiter", "stream"),
    "cgm_direction": ("n", "ch", "g", "scal", "it", "maxiter", "#part_pAp", "#part_rz", "#part_rr", "@z", "@p", "@x", "dt",
                      "stream"),
}
STARTS = ("cg_start", "cgm_start")
DIRECTIONS = ("cg_direction", "cgm_direction")
PER_ITERATION = ("cg_update", "cg_direction", "cg_xupdate", "cgm_direction")
OUT_PARTS = ("part_out",)            # partial OUTPUTS: sentinel everywhere, the call writes the local slots only
DTYPES = (np.float64, np.float32)

# the smallest shapes at which each code path changes; every chunk size with a grid of 1, 2 and 3 chunks
SHAPES = {
    2048: (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 6143),
    4096: (2049, 3073, 4095, 4096, 4097, 8195),       # 2049: the first step of the tail loop of hipk_pre::run
    8192: (2049, 8191, 8192, 8193, 16387),
}
SPECIAL_SHAPE = {2048: 4097, 4096: 8195, 8192: 16387}   # three chunks, a ragged last one (fp32: n % 4 = 1 or 3, fp64: odd)
G_KINDS = ("g=local", "g=local+5", "g=255", "g=256", "g=257", "g=2048")   # the fold has 8 rounds of 256
ITS = (3, 8, 5, 12)
GARBAGE = 0x5A5A5A5A5A5A5A5A
SENTINEL_PART = -7.25e77
SCAL_ALLOC = 14                      # words of hipk_cg_scal_bytes(): the 8 of the block, then fields of the whole solves


def g_value(kind, local):
    return {"g=local": local, "g=local+5": local + 5, "g=255": 255, "g=256": 256, "g=257": 257, "g=2048": 2048}[kind]


def _case(entry, dtype, ch, n, gk, it=0, maxiter=1000, block="running", kinds=(), tol=1e-5, atol=1e-7, x_null=False, split=False):
    local = sm.local_chunks(n, ch)
    tname = "f64" if dtype == np.float64 else "f32"
    kinds = set(kinds) | {gk}
    if min(n, ch) > sm.BASE_CHUNK:
        kinds.add("tail_loop")
    if n % sm.vec_width(dtype):
        kinds.add("ragged")
    if entry in PER_ITERATION:
        kinds.add(f"parity{it & 1}")
    cid = f"{entry}-{tname}-ch{ch}-n{n}-{gk[2:]}-it{it}-{block}" + (f"-max{maxiter}" if maxiter != 1000 else "") + ("-xnull" if x_null else "") + ("-split" if split else "")
    return types.SimpleNamespace(id=cid, entry=entry, dtype=dtype, ch=ch, n=n, g=g_value(gk, local), it=it, maxiter=maxiter,
                                 block=block, kinds=frozenset(kinds), tol=tol, atol=atol, x_null=x_null, split=split)


def _table():
    cases = []
    for entry in ARGS:
        for dtype in DTYPES:
            k = 0
            for ch, ns in SHAPES.items():
                for n in ns:
                    cases.append(_case(entry, dtype, ch, n, G_KINDS[k % len(G_KINDS)],
                                       it=ITS[k % len(ITS)] if entry in PER_ITERATION else 0))
                    k += 1
            ch = 4096
            n = SPECIAL_SHAPE[ch]
            gk = "g=local+5"
            if entry in PER_ITERATION:
                # it >= stop_it: no byte of any operand, partial array or the scalar block changes
                cases.append(_case(entry, dtype, ch, n, gk, it=6, block="stop==it", kinds={"noop_eq"}))
                cases.append(_case(entry, dtype, ch, n, gk, it=7, block="stop<it", kinds={"noop_gt"}))
                # sum(part_pAp) == 0: alpha is infinite
                cases.append(_case(entry, dtype, ch, n, gk, it=4, block="pAp=0", kinds={"nonfinite"}))
            if entry in DIRECTIONS:
                cases.append(_case(entry, dtype, ch, n, gk, it=9, maxiter=10, kinds={"maxiter_hit"}))
                cases.append(_case(entry, dtype, ch, n, gk, it=9, maxiter=11, kinds={"maxiter_minus1"}))
                cases.append(_case(entry, dtype, ch, n, gk, it=2, block="rr==atol2", kinds={"rr_eq"}))
                cases.append(_case(entry, dtype, ch, n, gk, it=3, block="rr==atol2+ulp", kinds={"rr_ulp"}))
            if entry in STARTS:
                cases.append(_case(entry, dtype, ch, n, gk, block="garbage", kinds={"garbage_block"}))
                cases.append(_case(entry, dtype, ch, n, gk, maxiter=0, block="garbage", kinds={"maxiter0", "garbage_block"}))
                cases.append(_case(entry, dtype, ch, n, gk, block="zero", tol=10.0, atol=0.0, kinds={"stopped_at_start"}))
                cases.append(_case(entry, dtype, ch, n, gk, block="rr0==tol", tol=0.5, atol=0.0, kinds={"eq_tol"}))
                cases.append(_case(entry, dtype, ch, n, gk, block="rr0==tol+ulp", tol=0.5, atol=0.0, kinds={"ulp_tol"}))
                cases.append(_case(entry, dtype, ch, n, gk, block="rr0==atol", tol=0.5, atol=48.0, kinds={"eq_atol"}))
                cases.append(_case(entry, dtype, ch, n, gk, block="rr0==atol+ulp", tol=0.5, atol=48.0, kinds={"ulp_atol"}))
            if entry == "cg_direction":
                for ch, n in SPECIAL_SHAPE.items():
                    # x == NULL: p only; and hipk_cg_xupdate followed by it: the x, p and block of the one call
                    cases.append(_case(entry, dtype, ch, n, gk, it=5, x_null=True, kinds={"x_null"}))
                    cases.append(_case(entry, dtype, ch, n, gk, it=4, split=True, kinds={"split"}))
    return cases


def _exact_parts(rng, g, target, ulp_up=False):
    """g nonzero partials whose fold is exactly `target` (a multiple of 2^-10 in [2^11, 2^12) or [2^13, 2^14)) in ANY summation
    order: all but slot 0 are multiples of 2^-10 of magnitude <= 1/8, so every intermediate sum is exact and stays in the binade
    of `target`; ulp_up adds one ulp of `target` to slot 0, which that binade carries along exactly."""
    part = rng.integers(1, 129, size=g).astype(np.float64) / 1024.0 * rng.choice([-1.0, 1.0], size=g)
    part[0] = target - float(np.sum(part[1:]))
    want = target
    if ulp_up:
        want = float(np.nextafter(target, np.inf))
        part[0] += want - target
    assert O.reduce_parts(part) == want and np.all(part != 0.0)
    return part


def inputs(case):
    """The operands of a case: vectors of n elements, partial arrays of 2048 slots, the scalar block."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    n, g, T = case.n, case.g, case.dtype
    vec, part = {}, {}
    for tok in ARGS[case.entry]:
        if tok[0] == "@":
            vec[tok[1:]] = rng.uniform(-1.0, 1.0, n).astype(T)
        elif tok[0] == "#":
            name = tok[1:]
            if name in OUT_PARTS:
                part[name] = np.full(sm.MAX_PARTS, SENTINEL_PART)
            else:
                # the g slots a call must fold (those beyond the local chunks included), then slots it must not read
                part[name] = rng.uniform(0.5, 1.5, sm.MAX_PARTS) * np.exp2(rng.integers(-3, 4, sm.MAX_PARTS))
    scal = rng.uniform(1.0, 2.0, SCAL_ALLOC)
    it, blk = case.it, case.block
    stop, sig = sm.stop_word(scal), sm.sig_word(scal)
    stop[0], sig[0] = sm.INT64_MAX, 0
    if case.entry in PER_ITERATION:
        scal[it & 1] = rng.uniform(0.5, 1.5)
        scal[(it + 1) & 1] = 123.456          # the other parity slot: a different value
        scal[sm.ATOL2] = 1e-30
    if blk == "stop==it":
        stop[0] = it
    elif blk == "stop<it":
        stop[0] = it - 3
    elif blk == "pAp=0":
        part["part_pAp"][:g] = 0.0
        part["part_pAp"][0], part["part_pAp"][g - 1] = 1.0, -1.0
        assert O.reduce_parts(part["part_pAp"][:g]) == 0.0
    elif blk in ("rr==atol2", "rr==atol2+ulp"):
        rr = O.reduce_parts(part["part_rr"][:g])
        scal[sm.ATOL2] = rr if blk == "rr==atol2" else float(np.nextafter(rr, -np.inf))
    elif blk == "garbage":
        scal.view(np.uint64)[:] = GARBAGE
    elif blk == "zero":
        scal[:] = 0.0
    elif blk.startswith("rr0=="):
        # tol = 0.5: tol^2 <b,b> = 2304 with <b,b> = 9216; atol = 48: atol^2 = 2304 with tol^2 <b,b> = 16
        part["part_rr"][:g] = _exact_parts(rng, g, 2304.0, ulp_up=blk.endswith("+ulp"))
        if "atol" not in blk:
            part["part_bb"][:g] = _exact_parts(rng, g, 9216.0)
        else:
            assert 0.25 * O.reduce_parts(part["part_bb"][:g]) < 2304.0
        scal.view(np.uint64)[:] = GARBAGE
    return types.SimpleNamespace(vec=vec, part=part, scal=scal)


def call_args(case, resolve_vec, resolve_part, scal):
    """The positional arguments of the case's entry point without dtype and stream (the mirror's signature)."""
    out = []
    for tok in ARGS[case.entry]:
        if tok in ("dt", "stream"):
            continue
        if tok[0] == "@":
            out.append(None if (tok == "@x" and case.x_null) else resolve_vec(tok[1:]))
        elif tok[0] == "#":
            out.append(resolve_part(tok[1:]))
        elif tok == "scal":
            out.append(scal)
        else:
            out.append({"n": case.n, "ch": case.ch, "g": case.g, "it": case.it, "maxiter": case.maxiter, "tol": case.tol,
                        "atol": case.atol}[tok])
    return out


def expected(case, inp, mirror=sm.TRUE):
    """Every output of the call according to `mirror` (the split form is one hipk_cg_direction)."""
    vec = {k: v.copy() for k, v in inp.vec.items()}
    part = {k: v.copy() for k, v in inp.part.items()}
    scal = inp.scal.copy()
    getattr(mirror, case.entry)(*call_args(case, vec.__getitem__, part.__getitem__, scal))
    return outputs(vec, part, scal)


def outputs(vec, part, scal):
    out = {f"vec:{k}": v for k, v in vec.items()}
    out.update({f"part:{k}": v for k, v in part.items()})
    out["scal"] = scal[:sm.SCAL_WORDS]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(case, got, want):
    """Names of the outputs that differ: bitwise, but NaN equal to NaN in the one non-finite kind."""
    bad = []
    for k in want:
        g, w = got[k], want[k]
        if "nonfinite" in case.kinds and k != "scal":
            ok = g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)
        else:
            ok = g.dtype == w.dtype and np.array_equal(bits(g), bits(w))
        if not ok:
            bad.append(k)
    return bad


CASES = _table()
