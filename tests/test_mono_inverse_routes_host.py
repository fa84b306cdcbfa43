"""Which kernel the Monotonic inverse launches, asked of the library itself (gnf_monotonic_inv_route: host arithmetic, no
GPU) for every row of tests/mono_inverse_cases.py -- the table tests/test_gpu_mono_inverse.py runs against fp64.  A row
claims a kernel family, its template arguments, the workgroup size and the grid; a threshold of inv_route that moves puts a
pinned shape on another route and fails here instead of silently changing what the GPU test covers.

Branches of inv_route / persistent_route that no sane shape reaches, and that the table therefore leaves out:
  * WM = 0 (weights from L2) anywhere but HT = 16: the image of a net of H <= 160 misses the 150 KB of LDS it may take
    only with more than one matrix (then one is resident at a time, WM = 2) or with a conditioning width in the
    thousands.  So mono_fwd_x_k<3, EX, 0, INV> and mono_inv_split_x_k<3, EX, 0, EPG> (peeled nets: 3 matrices of 18 KB),
    mono_inv_split_k<2 | 4 | 7 | 10, 0, EPG> and mono_fwd_k<2 | 4 | 7 | 10, 0, true> stay unpinned.
  * mono_fwd_k<2 | 4, 2, true>: up to six matrices of 5 / 18 KB fit beside any first layer of a sane width.
  * mono_fwd_k<16, 2, true>: one 256 x 260 matrix is 260 KB, never resident.  mono_fwd_k<16, 1, true> needs the
    one-hidden-layer net at S < 7 or n > 8192; its image plan is the <16, 1, EPG> row's.
  * mono_inv_ks_x_k<3, EX, 2, 12>: with two elements per workgroup S <= 31 gives at most 6 wavefronts -- unreachable, and
    no longer instantiated (EDGES has the 6-wavefront launch).
  * L.c = 0: the conditioner's output always holds h0, so the first layer has at least one conditioning column
    (cond_size 1 is L.c = 1: IntegrandNet's first layer is 1 + cond_size wide)."""
import ctypes

import pytest

from mono_inverse_cases import ROWS, EDGES, case_id

EINVAL, ESHAPE = -1, -2


def _net(hidden, c):
    """a gnf_mono_net of dims alone: the query reads no parameter"""
    from gnf_hip import abi
    net = abi.MonoNet()
    net.nl = len(hidden) + 1
    for l, w in enumerate([1 + c] + list(hidden) + [1]):
        net.dims[l] = w
    return net


def query(hidden, c, S, B, d, size=256):
    from gnf_hip import abi
    buf = ctypes.create_string_buffer(size)
    rc = abi.load().gnf_monotonic_inv_route(ctypes.byref(_net(hidden, c)), S, B, d, buf, size)
    return rc, buf.value.decode()


def parse(line):
    """'family<K=v,...> block=.. grid=.. lds=..' -> (family, {K: v}, {block, grid, lds})"""
    head, rest = line.split("> ")
    family, args = head.split("<")
    return (family, {k: int(v) for k, v in (kv.split("=") for kv in args.split(","))},
            {k: int(v) for k, v in (kv.split("=") for kv in rest.split())})


@pytest.mark.parametrize("row", ROWS + EDGES, ids=[case_id(r) for r in ROWS] + ["edge-" + case_id(r) for r in EDGES])
def test_row_takes_the_route_it_claims(row):
    hidden, c, S, B, d, template, block, grid = row
    rc, line = query(hidden, c, S, B, d)
    assert rc == 0, rc
    family, args, launch = parse(line)
    assert line.split(" ")[0] == template, line
    assert (launch["block"], launch["grid"]) == (block, grid), line
    assert launch["block"] % 64 == 0 and 0 <= launch["lds"] <= 160 * 1024
    # a kernel that keeps the weight image in LDS asks for LDS, one that reads it from L2 for next to none
    wm = args.get("WM", 1)
    assert (launch["lds"] > 4096) == (wm != 0), line


# what the rows must reach between them: every value of every axis of inv_route that a sane shape can reach (the module
# docstring has the rest)
REACHABLE = {
    ("mono_inv_split_k", "HT"): {2, 4, 7, 10, 16}, ("mono_inv_split_k", "WM"): {0, 1}, ("mono_inv_split_k", "EPG"): {4, 16},
    ("mono_inv_split_x_k", "HM"): {3}, ("mono_inv_split_x_k", "EX"): {2, 3}, ("mono_inv_split_x_k", "WM"): {1},
    ("mono_inv_split_x_k", "EPG"): {4, 16},
    ("mono_inv_ks_x_k", "HM"): {3}, ("mono_inv_ks_x_k", "EX"): {2, 3}, ("mono_inv_ks_x_k", "epg"): {2, 4},
    ("mono_inv_ks_x_k", "waves"): {8, 12},
    ("mono_fwd_k", "HT"): {2, 4, 7, 10, 16}, ("mono_fwd_k", "WM"): {0, 1, 2}, ("mono_fwd_k", "INV"): {1},
    ("mono_fwd_x_k", "HM"): {3}, ("mono_fwd_x_k", "EX"): {2, 3}, ("mono_fwd_x_k", "WM"): {1}, ("mono_fwd_x_k", "INV"): {1},
}


def test_rows_reach_every_reachable_axis_value():
    seen, templates = {}, set()
    for hidden, c, S, B, d, template, _, _ in ROWS:           # the rows the GPU test runs; EDGES add none
        rc, line = query(hidden, c, S, B, d)
        assert rc == 0
        family, args, _ = parse(line)
        templates.add(line.split(" ")[0])
        for k, v in args.items():
            seen.setdefault((family, k), set()).add(v)
    assert seen == REACHABLE, {k: seen.get(k, set()) ^ REACHABLE.get(k, set()) for k in set(seen) | set(REACHABLE)
                               if seen.get(k) != REACHABLE.get(k)}
    # ... and the combinations the issue of record names: both EPG of both split kernels on both kinds of image, the
    # persistent inverse with the image resident, swapped and in L2, both EX on every peeled family
    for t in ("mono_inv_split_k<HT=2,WM=1,EPG=16>", "mono_inv_split_k<HT=7,WM=1,EPG=16>", "mono_inv_split_k<HT=16,WM=0,EPG=4>",
              "mono_inv_split_k<HT=16,WM=1,EPG=4>", "mono_fwd_k<HT=16,WM=0,INV=1>", "mono_fwd_k<HT=7,WM=2,INV=1>",
              "mono_fwd_k<HT=2,WM=1,INV=1>", "mono_fwd_x_k<HM=3,EX=3,WM=1,INV=1>", "mono_inv_split_x_k<HM=3,EX=3,WM=1,EPG=4>",
              "mono_inv_split_x_k<HM=3,EX=3,WM=1,EPG=16>", "mono_inv_ks_x_k<HM=3,EX=3,epg=2,waves=8>",
              "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=12>"):
        assert t in templates, t
    # the thresholds on n and S: the table holds shapes on both sides of each (ngroups 255 | 256, 512 | 513; S 6 | 7, 31 | 32;
    # n 512 | 513) and the grid-stride second trip
    ns = {(S, -(-B * d // 16)) for _, _, S, B, d, _, _, _ in ROWS + EDGES}
    assert {g for _, g in ns} >= {3, 255, 256, 512, 513, 2051} and {S for S, _ in ns} >= {3, 6, 7, 21, 31, 32, 70}
    assert {B * d for _, _, _, B, d, _, _, _ in ROWS + EDGES} >= {512, 513, 4083, 32802}


def test_epg2_never_needs_twelve_wavefronts():
    """the dispatch drops mono_inv_ks_x_k<3, EX, 2, 12>: over every S the two-step kernel takes (7..31) and every n that puts
    two elements in a workgroup, the launch has at most 6 wavefronts"""
    for S in range(7, 32):
        for n in (1, 2, 511, 512):
            rc, line = query([50, 50, 50], 30, S, n, 1)
            family, args, launch = parse(line)
            assert rc == 0 and family == "mono_inv_ks_x_k" and args["epg"] == 2 and args["waves"] == 8, line
            assert launch["block"] == 64 * ((3 * (S + 1) + 1) // 2 * 2 + 15 >> 4) <= 64 * 6, line


def test_query_refuses_what_the_entry_point_refuses():
    from gnf_hip import abi
    lib = abi.load()
    buf = ctypes.create_string_buffer(256)
    ok = _net([20, 20], 5)
    assert lib.gnf_monotonic_inv_route(ctypes.byref(ok), 20, 11, 3, buf, 256) == 0
    for S, B, d in ((0, 11, 3), (20, -1, 3), (20, 11, 0)):
        assert lib.gnf_monotonic_inv_route(ctypes.byref(ok), S, B, d, buf, 256) == EINVAL
    assert lib.gnf_monotonic_inv_route(ctypes.byref(ok), 20, 11, 3, None, 256) == EINVAL
    assert lib.gnf_monotonic_inv_route(ctypes.byref(ok), 20, 11, 3, buf, 0) == EINVAL
    assert lib.gnf_monotonic_inv_route(ctypes.byref(ok), 20, 11, 3, buf, 20) == EINVAL       # line does not fit
    assert lib.gnf_monotonic_inv_route(None, 20, 11, 3, buf, 256) == ESHAPE
    assert lib.gnf_monotonic_inv_route(ctypes.byref(_net([257, 20], 5)), 20, 11, 3, buf, 256) == ESHAPE   # wider than 16 tiles
    one = abi.MonoNet()
    one.nl, one.dims[0], one.dims[1] = 1, 6, 1
    assert lib.gnf_monotonic_inv_route(ctypes.byref(one), 20, 11, 3, buf, 256) == ESHAPE     # no hidden layer
    two_out = _net([20, 20], 5)
    two_out.dims[3] = 2
    assert lib.gnf_monotonic_inv_route(ctypes.byref(two_out), 20, 11, 3, buf, 256) == ESHAPE
    # an empty batch is a valid call that launches nothing
    assert lib.gnf_monotonic_inv_route(ctypes.byref(ok), 20, 0, 3, buf, 256) == 0 and buf.value == b""
    # the shape check comes before the argument check, as in the entry points
    assert lib.gnf_monotonic_inv_route(None, 0, 11, 3, buf, 256) == ESHAPE

