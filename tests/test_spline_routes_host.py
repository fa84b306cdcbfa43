"""How the Spline kernels run a problem, asked of the library itself (gnf_spline_route: host arithmetic from the function
the three entry points launch from, no GPU) for every case of tests/spline_cases.py -- the table
tests/test_gpu_spline_long.py runs against fp64.  A case claims the forward's rows per workgroup, chunks and grid and the
staging routes of h and gh; a threshold of gnf_spline.hip that moves puts a pinned case on another route and fails here
instead of silently changing what the GPU test covers."""
import ctypes
import os
import re

import pytest

import spline_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2
FWD, BWD, INV = 0, 1, 2
ALIGNED = 0x7f0000001000                    # an address on the 16-byte grid; never dereferenced


def route(which, h, hs, K, B, d, gh=None, gs=(0, 0, 0), scatter=0, size=256):
    """(rc, line); hs = (sb, sd, sc, h_c)"""
    from gnf_hip import abi
    buf = ctypes.create_string_buffer(size)
    rc = abi.load().gnf_spline_route(which, h, hs[0], hs[1], hs[2], hs[3], K, B, d, gh, gs[0], gs[1], gs[2], scatter, buf, size)
    return rc, buf.value.decode()


def parse(line):
    """'kernel key=value ...' -> (kernel, {key: value}), integers where they are"""
    head, *rest = line.split(" ")
    return head, {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (kv.split("=") for kv in rest)}


def case_routes(case, k=0):
    """the three lines of a case whose h (and gh) start 4 k bytes past a 16-byte boundary"""
    B, d, K, layout = case
    hs, gs = SC.h_and_gh_strides(layout, B, d, K)
    at = ALIGNED + 4 * k
    out = []
    for which in (FWD, BWD, INV):
        rc, line = route(which, at, hs, K, B, d, gh=at if which == BWD else None, gs=gs)
        assert rc == 0, (case, which, rc)
        out.append(parse(line))
    return out


def lds(K, red):
    pitch = (5 * K - 1) | 1
    return 4 * ((128 * pitch + 3) & ~3) + (16 * 128 if red else 0)


# ------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_case_takes_the_route_it_claims(case):
    B, d, K, layout = case
    (fk, f), (bk, b), (ik, i) = case_routes(case)
    assert (fk, bk, ik) == ("spline_fwd_k", "spline_bwd_k", "spline_inv_k")
    want = parse("x " + SC.SHAPES[(B, d)])[1]
    assert {k: f[k] for k in want} == want, f
    h_route, gh_route = SC.LAYOUTS[layout]
    if d == 1 and layout in ("made", "dmajor"):
        gh_route = b["gh"]                   # the stride of a dimension of size one is torch's to choose: no claim
    assert f["h"] == b["h"] == i["h"] == h_route and b["gh"] == gh_route, (f, b)
    # the element tiles of the backward and the inverse, whatever the rows are
    tiles = -(-B * d // SC.KTILE)
    for r in (b, i):
        assert (r["rows_per_wg"], r["chunks"], r["grid"]) == (0, 1, tiles), r
    assert i["out"] == "plain"
    assert f["lds"] == lds(K, True) and b["lds"] == i["lds"] == lds(K, False) and f["lds"] <= 160 * 1024
    # a tile of 128 elements starts on the 16-byte grid whenever the tensor does: all or none
    assert b["tiles16"] == i["tiles16"] == (tiles if h_route == "span16" else 0)
    assert b["gtiles16"] == (tiles if gh_route == "span16" else 0)
    assert 0 <= f["tiles16"] <= f["grid"] * f["chunks"] and (f["tiles16"] > 0) == (h_route == "span16")
    if case in SC.MIXED:
        assert (f["tiles16"], f["grid"] * f["chunks"]) == SC.MIXED[case], f


def test_hand_computed_lines():
    c23 = (23 * 129, 23, 1, 23)
    assert route(FWD, ALIGNED, c23, 8, 3, 129) == \
        (0, "spline_fwd_k rows_per_wg=1 chunks=2 grid=3 lds=22016 h=span16 tiles16=2")      # pitch 39: 4 128 39 + 2048
    assert route(FWD, ALIGNED + 4, c23, 8, 3, 129) == \
        (0, "spline_fwd_k rows_per_wg=1 chunks=2 grid=3 lds=22016 h=span4 tiles16=0")
    assert route(BWD, ALIGNED, c23, 8, 3, 129, gh=ALIGNED + 8, gs=c23[:3]) == \
        (0, "spline_bwd_k rows_per_wg=0 chunks=1 grid=4 lds=19968 h=span16 tiles16=4 gh=span4 gtiles16=0")
    assert route(INV, ALIGNED, (23 * 129, 1, 129, 23), 8, 3, 129, scatter=1) == \
        (0, "spline_inv_k rows_per_wg=0 chunks=1 grid=4 lds=19968 h=rows tiles16=0 out=cols")       # MADE's view
    assert route(FWD, ALIGNED, (5, 5, 1, 5), 2, 300, 1) == \
        (0, "spline_fwd_k rows_per_wg=128 chunks=1 grid=3 lds=6656 h=span16 tiles16=3")      # pitch 9: 4 1152 + 2048
    assert route(FWD, ALIGNED, (95 * 3072, 95, 1, 95), 32, 1, 3072) == \
        (0, "spline_fwd_k rows_per_wg=1 chunks=24 grid=1 lds=83456 h=span16 tiles16=24")     # pitch 159: 4 20352 + 2048
    # the edge of the span form: sd = 4096 | 4097, and sd < C (overlapping rows) is no span either
    assert parse(route(FWD, ALIGNED, (4096 * 64, 4096, 1, 23), 8, 5, 64)[1])[1]["h"] == "span16"
    assert parse(route(FWD, ALIGNED, (4097 * 64, 4097, 1, 23), 8, 5, 64)[1])[1]["h"] == "rows"
    assert parse(route(FWD, ALIGNED, (22 * 64, 22, 1, 23), 8, 5, 64)[1])[1]["h"] == "rows"
    assert parse(route(FWD, ALIGNED, (23 * 64 + 1, 23, 1, 23), 8, 5, 64)[1])[1]["h"] == "rows"
    # both sides of the thresholds on d
    for d, rt, ch in ((63, 2, 1), (64, 2, 1), (65, 1, 1), (128, 1, 1), (129, 1, 2), (256, 1, 2), (257, 1, 3)):
        f = parse(route(FWD, ALIGNED, (23 * d, 23, 1, 23), 8, 7, d)[1])[1]
        assert (f["rows_per_wg"], f["chunks"], f["grid"]) == (rt, ch, -(-7 // rt)), (d, f)


def test_table_reaches_every_route():
    """over the table gnf_spline_route reports: rows_per_wg > 1 and == 1; chunks == 1 and > 1; a ragged last chunk and an
    exactly full one; a forward with SOME tiles on the 16-byte path; each of span16 / span4 / rows for h; a backward whose
    h and gh take different routes; and the reduction loop's trip counts 1, 3 and 8"""
    seen = {"rt": set(), "chunks": set(), "ragged": set(), "h": set(), "mixed": 0, "h_gh": set(), "trips": set(),
            "ragged_wg": 0, "short_tile": 0}
    for case in SC.CASES:
        B, d, K, layout = case
        (_, f), (_, b), _ = case_routes(case)
        seen["rt"].add(f["rows_per_wg"] > 1)
        seen["chunks"].add(f["chunks"] > 1)
        if f["chunks"] > 1:
            assert f["chunks"] == -(-d // SC.KTILE)
            seen["ragged"].add(d % SC.KTILE != 0)
        seen["h"].add(f["h"])
        seen["mixed"] += 0 < f["tiles16"] < f["grid"] * f["chunks"]
        seen["h_gh"].add((b["h"], b["gh"]))
        if f["rows_per_wg"] > 1:
            seen["trips"].add(-(-min(f["rows_per_wg"], B) * 8 // SC.KTILE))
            seen["ragged_wg"] += B % f["rows_per_wg"] != 0
        seen["short_tile"] += f["rows_per_wg"] == 1 and d < SC.KTILE
    for case in SC.ALIGN:
        for k in (1, 2, 3):
            (_, f), (_, b), (_, i) = case_routes(case, k)
            seen["h"].add(f["h"])
            span = SC.LAYOUTS[case[3]][0] != "rows"
            assert (f["h"], b["h"], i["h"], b["gh"]) == (("span4",) * 4 if span else ("rows",) * 4), (case, k)
            assert f["tiles16"] == b["tiles16"] == b["gtiles16"] == i["tiles16"] == 0 and f["chunks"] == 2
    assert seen["rt"] == seen["chunks"] == seen["ragged"] == {False, True}, seen
    assert seen["h"] == {"span16", "span4", "rows"}, seen
    assert seen["mixed"] > 0 and seen["ragged_wg"] > 0 and seen["short_tile"] > 0
    assert seen["trips"] >= {1, 3, 8}, seen
    assert {("rows", "span16"), ("span16", "span4"), ("span16", "span16"), ("rows", "rows")} <= seen["h_gh"], seen
    assert any(h != g for h, g in seen["h_gh"])
    # every layout and every shape of the table's header is in it, the slice layouts at B <= 3 only
    assert {c[3] for c in SC.CASES} == set(SC.LAYOUTS) and {c[:2] for c in SC.CASES} == set(SC.SHAPES)
    assert {c[2] for c in SC.CASES} == set(SC.BINS)
    assert all(c[0] <= 3 for c in SC.CASES if c[3].startswith("slice"))
    assert all(c in SC.CASES for c in SC.MIXED) and all(c in SC.CASES for c in SC.ALIGN)


# ------------------------------------------------------------------------------------------------------- the query itself
def test_query_refuses_what_the_entry_points_refuse():
    ok = (69, 23, 1, 23)
    for which in (FWD, BWD, INV):
        gh = ALIGNED if which == BWD else None
        q = lambda hs=ok, K=8, B=4, d=3, h=ALIGNED, gh=gh, **kw: route(which, h, hs, K, B, d, gh=gh, gs=ok[:3], **kw)[0]
        assert q() == 0
        assert q(K=1) == EINVAL and q(K=33, hs=(294, 98, 1, 98)) == EINVAL
        assert q(B=-1) == EINVAL and q(d=0) == EINVAL
        assert q(hs=(66, 22, 1, 22)) == ESHAPE                   # h too narrow
        assert q(h=None) == EINVAL                               # NULL with B > 0 ...
        assert q(h=None, gh=None, B=0) == 0                      # ... and with an empty batch
        assert q(K=1, hs=(66, 22, 1, 2)) == EINVAL               # the argument check comes before the shape check
        assert q(B=1 << 37, d=1) == 0 and q(B=1 << 40, d=1) == ESHAPE    # 2^30 workgroups; 2^33
        assert q(B=1 << 40, d=128) == ESHAPE
        assert q(size=20) == EINVAL                              # the line does not fit
        rc, line = route(which, ALIGNED, ok, 8, 0, 3, gh=gh, gs=ok[:3])
        assert (rc, line) == (0, "")                             # an empty batch launches nothing
    assert route(BWD, ALIGNED, ok, 8, 4, 3, gh=None)[0] == EINVAL
    from gnf_hip import abi
    lib = abi.load()
    buf = ctypes.create_string_buffer(256)
    assert lib.gnf_spline_route(3, ALIGNED, 69, 23, 1, 23, 8, 4, 3, None, 0, 0, 0, 0, buf, 256) == EINVAL
    assert lib.gnf_spline_route(-1, ALIGNED, 69, 23, 1, 23, 8, 4, 3, None, 0, 0, 0, 0, buf, 256) == EINVAL
    assert lib.gnf_spline_route(0, ALIGNED, 69, 23, 1, 23, 8, 4, 3, None, 0, 0, 0, 0, None, 256) == EINVAL
    assert lib.gnf_spline_route(0, ALIGNED, 69, 23, 1, 23, 8, 4, 3, None, 0, 0, 0, 0, buf, 0) == EINVAL


def test_entry_points_and_query_refuse_alike():
    """every refusal above, put to the entry point itself (pointers never dereferenced: each call is refused or empty)"""
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)

    def entry(which, K, hc, B, d, h):
        if which == FWD:
            return lib.gnf_spline_fwd(p, h, d * hc, hc, 1, hc, K, 3., p, p, p, p, B, d, None)
        if which == BWD:
            return lib.gnf_spline_bwd(p, h, d * hc, hc, 1, hc, K, 3., p, p, p, p, p, p, d * hc, hc, 1, B, d, None)
        return lib.gnf_spline_inv(p, h, d * hc, hc, 1, hc, K, 3., p, None, 0, B, d, None)
    for which in (FWD, BWD, INV):
        for K, hc, B, d, h in ((1, 23, 4, 3, p), (33, 98, 4, 3, p), (8, 23, -1, 3, p), (8, 23, 4, 0, p), (8, 22, 4, 3, p),
                               (8, 23, 4, 3, None), (8, 23, 0, 3, None), (1, 2, 4, 3, p), (8, 23, 1 << 40, 128, p)):
            rc = route(which, h.value if h is not None else None, (d * hc, hc, 1, hc), K, B, d, gh=64, gs=(d * hc, hc, 1))[0]
            assert rc == entry(which, K, hc, B, d, h) and rc <= 0, (which, K, hc, B, d)


def test_one_decision_function():
    """the source itself: the entry points and the query take RT, nchunk, grid, LDS size and layouts from spline_plan, and
    nothing else in the file computes them"""
    src = open(os.path.join(ROOT, "graphical-normalizing-flows_amd", "gnf_hip", "csrc", "gnf_spline.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)
    host = src[src.index('extern "C"'):]
    bodies = re.findall(r"\nint (gnf_spline_\w+)\([^)]*\) \{\n(.*?)\n\}\n", host, flags=re.S)
    assert [n for n, _ in bodies] == ["gnf_spline_fwd", "gnf_spline_bwd", "gnf_spline_inv", "gnf_spline_route"]
    for name, body in bodies:
        assert body.count("spline_plan(") == 1, name
        for word in ("make_lay", "lds_bytes", "kTile /", "/ kTile", "HLay"):
            assert word not in body, (name, word)
        if name != "gnf_spline_route":
            launch = body[body.index("gnf_launch_lds("):]
            assert "dim3((unsigned)p.grid)" in launch and "p.lds" in launch and "p.l," in launch, name
    assert "p.RT)" in bodies[0][1] and "p.gl," in bodies[1][1]
    assert src.count("make_lay(") == 3 and src.count("lds_bytes(") == 2          # their definitions and spline_plan's uses


def test_symbol_declared_and_bound():
    from gnf_hip import abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnf_hip.h")).read(), flags=re.S)
    m = re.search(r"\bgnf_spline_route\s*\(([^)]*)\)", header)
    assert m is not None and hasattr(abi.load(), "gnf_spline_route")
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES["gnf_spline_route"][1]) == 16
    assert (abi.SPLINE_FWD, abi.SPLINE_BWD, abi.SPLINE_INV) == (FWD, BWD, INV)
    assert abi.ABI_VERSION == 11 and abi.load().gnf_abi_version() == 11
