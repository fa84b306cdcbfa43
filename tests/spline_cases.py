"""Case table of the Spline kernels' host decisions (spline_plan of gnf_hip/csrc/gnf_spline.hip), shared by
tests/test_spline_routes_host.py (the route each case claims, asked of gnf_spline_route: no GPU) and
tests/test_gpu_spline_long.py (the kernels on that route against fp64).

A case is (B, d, K, layout).  What it is in the table for is claimed per SHAPE (the forward's rows per workgroup, chunks of a
row and grid) and per LAYOUT (the staging route of h, and of the gh that ops.SplineFn.backward allocates for it); the host
test holds every claim against the line the library prints.  kTile = 128, C = 3 K - 1.

The shapes are the smallest that can still go wrong:
    (300, 1)   RT = 128, eight trips of the reduction loop, ragged last workgroup (300 = 2 128 + 44)
    (70, 3)    RT = 42, ragged last workgroup
    (5, 64)    RT = 2, the last workgroup holds one row
    (5, 65)    the first RT = 1, n < kTile
    (3, 127), (3, 128), (3, 129)   the chunk boundary: 129 leaves a chunk of one lane, and 129 23 % 4 != 0 puts rows 1 and
               2 on the dword span while row 0 is on the 16-byte span
    (2, 300), (2, 784), (1, 3072)  several full chunks and a ragged one (3072: 24 full ones); the MNIST and CIFAR widths
"""
import torch

KTILE = 128
T, SCALE = 3., 1.                           # the tail and the scale of h: one of each (the short rows have the others)

# (B, d) -> the forward's claim, as gnf_spline_route prints it
SHAPES = {
    (300, 1): "rows_per_wg=128 chunks=1 grid=3",
    (70, 3): "rows_per_wg=42 chunks=1 grid=2",
    (5, 64): "rows_per_wg=2 chunks=1 grid=3",
    (5, 65): "rows_per_wg=1 chunks=1 grid=5",
    (3, 127): "rows_per_wg=1 chunks=1 grid=3",
    (3, 128): "rows_per_wg=1 chunks=1 grid=3",
    (3, 129): "rows_per_wg=1 chunks=2 grid=3",
    (2, 300): "rows_per_wg=1 chunks=3 grid=2",
    (2, 784): "rows_per_wg=1 chunks=7 grid=2",
    (1, 3072): "rows_per_wg=1 chunks=24 grid=1",
}
BINS = (2, 8, 32)                           # C = 5, 23, 95: the smallest and the largest

# layout -> (route of h, route of the gh the backward allocates), on a 16-byte aligned allocation.
#   contig     [B, d, C]
#   made       MADE's permuted view of [B, C, d]
#   wide       [B, d, C + 2]: components the normalizer does not read; stage_out goes by dwords (sd != C)
#   slice<sd>  big[:, :, :C] of [B, d, sd]: 513 > 4 kTile (de = 0 in the span walkers), 4096 the last span width, 4097 the
#              first that falls to rows with sc == 1
#   rowpad     big[:, :d] of [B, d + 1, C]: sb != d sd
#   dmajor     [d, B, C] permuted to [B, d, C]
# A view that is not dense gets a CONTIGUOUS gh from torch.empty_like: the backward stages in and out on different routes.
LAYOUTS = {
    "contig": ("span16", "span16"),
    "made": ("rows", "rows"),
    "wide": ("span16", "span4"),
    "slice513": ("span16", "span16"),
    "slice4096": ("span16", "span16"),
    "slice4097": ("rows", "span16"),
    "rowpad": ("rows", "span16"),
    "dmajor": ("rows", "rows"),
}
OLD_LAYOUTS = ("contig", "made", "wide")    # the three of tests/test_gpu_spline.py


def geometry(layout, B, d, C):
    """(shape of the allocation, function taking the allocation to the [B, d, >= C] view the kernels are handed)"""
    if layout == "contig":
        return (B, d, C), lambda big: big
    if layout == "made":
        return (B, C, d), lambda big: big.permute(0, 2, 1)
    if layout == "wide":
        return (B, d, C + 2), lambda big: big
    if layout.startswith("slice"):
        return (B, d, int(layout[5:])), lambda big: big[:, :, :C]
    if layout == "rowpad":
        return (B, d + 1, C), lambda big: big[:, :d]
    if layout == "dmajor":
        return (d, B, C), lambda big: big.permute(1, 0, 2)
    raise KeyError(layout)


def h_and_gh_strides(layout, B, d, K):
    """((sb, sd, sc, h_c) of the view, (sb, sd, sc) of the gh of ops.SplineFn.backward) from torch's own stride rules, on
    the meta device: nothing is allocated"""
    C = 3 * K - 1
    shape, view = geometry(layout, B, d, C)
    h = view(torch.empty(shape, device="meta"))
    gh = torch.empty_like(h) if h.shape[2] == C else torch.zeros_like(h)
    return tuple(h.stride()) + (h.shape[2],), tuple(gh.stride())


# the slice layouts at B <= 3 only, so that the largest operand stays a few MB (3 129 4097 floats = 6.3 MB)
EXTRA = [
    (3, 129, 2, "slice513"), (3, 129, 8, "slice513"), (3, 129, 32, "slice513"), (3, 128, 8, "slice513"), (2, 784, 8, "slice513"),
    (3, 129, 8, "slice4096"), (3, 129, 32, "slice4096"), (3, 127, 8, "slice4096"),
    (3, 129, 8, "slice4097"), (3, 129, 32, "slice4097"), (3, 128, 2, "slice4097"),
    (300, 1, 8, "rowpad"), (70, 3, 8, "rowpad"), (5, 64, 8, "rowpad"), (5, 65, 2, "rowpad"), (3, 129, 8, "rowpad"),
    (2, 300, 32, "rowpad"),
    (300, 1, 2, "dmajor"), (70, 3, 8, "dmajor"), (5, 65, 8, "dmajor"), (3, 129, 32, "dmajor"), (2, 784, 8, "dmajor"),
]
CASES = [(B, d, K, lay) for (B, d) in SHAPES for K in BINS for lay in OLD_LAYOUTS] + EXTRA

# forward tiles on the 16-byte path out of grid x chunks, where that is not all of them: a workgroup's span starts at
# element e0 = (rows before it) d, and (e0 sd) % 4 decides -- hand-computed
MIXED = {
    (3, 129, 8, "contig"): (2, 6),          # 129 23 = 2967 = 3 (mod 4), 258 23 = 2 (mod 4): row 0 alone, two chunks
    (3, 129, 2, "contig"): (2, 6),          # 129 5 = 1 (mod 4)
    (3, 129, 32, "contig"): (2, 6),         # 129 95 = 3 (mod 4)
    (3, 127, 8, "contig"): (1, 3),          # 127 23 = 1 (mod 4)
    (5, 65, 8, "contig"): (2, 5),           # 65 23 = 3 (mod 4): rows 0 and 4
    (3, 129, 8, "slice513"): (1 * 2, 6),    # 129 513 = 1 (mod 4)
    (3, 129, 8, "wide"): (2, 6),            # 129 25 = 1 (mod 4)
    (70, 3, 8, "contig"): (1, 2),           # 42 3 23 = 2898 = 2 (mod 4)
    (300, 1, 8, "contig"): (3, 3),          # 128 23: every workgroup
    (3, 128, 8, "contig"): (3, 3),
    (2, 784, 8, "contig"): (14, 14),
    (3, 129, 8, "slice4096"): (6, 6),       # sd a multiple of 4: every tile
}

# the dword-alignment cases of tests/test_gpu_spline.py on a chunked row: (B, d, K, layout), at 4 k bytes past a 16-byte
# boundary, k = 1..3 -- a span layout then has no tile on the 16-byte path (h=span4 tiles16=0)
ALIGN = [(3, 129, 8, "contig"), (3, 129, 8, "made")]


def case_id(c):
    return "%dx%d-K%d-%s" % c
