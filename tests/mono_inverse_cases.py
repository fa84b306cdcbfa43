"""Case table of the Monotonic inverse's dispatch (inv_route of gnf_hip/csrc/gnf_monotonic.hip), shared by
tests/test_mono_inverse_routes_host.py (the route each row claims, no GPU) and tests/test_gpu_mono_inverse.py (the kernel of
that route against fp64).

A row is (hidden, cond_size, S, B, d, template, block, grid): the integrand net, the node count, the [B, d] problem and the
route claimed for it -- the kernel family with its template arguments as gnf_monotonic_inv_route prints them, the workgroup
size and the grid.  n = B d; d = 3 where 3 divides n and 5 or 7 otherwise, so that e / d and e % d of the scattered store
and of h's strides matter.  The shapes are the smallest that reach each branch:

    ngroups = ceil(n / 16):  3 (n = 33, 35), 33 (515), 256 (4083: the first count that is not "quarter", ragged by 3),
                             513 (8195: the first past the split kernels), 2051 (32802: 513 workgroups wanted, 512 run, so
                             workgroup 0 makes a second grid-stride trip, ragged by 2)
    S:  3 (< 7: persistent), 7 (one wavefront), 8, 20 (even: S + 1 nodes, so the last pair is a half pair, k1 > S), 21 (odd:
        every pair full), 31 (the last of the two-step kernel), 32, 40, 70 (more node pairs than slots: a second kb trip)
"""

# workgroup sizes are 64 x wavefronts
ROWS = [
    # ---- mono_inv_split_k: the split-node inverse of every net that is not [49..51]^k
    ([20, 20], 5, 20, 11, 3, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 192, 9),       # 11 pairs on 3 x 4 slots: one idle, a half pair
    ([20, 20], 5, 7, 11, 3, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 64, 9),         # 4 pairs, one wavefront
    ([20, 20], 5, 21, 11, 3, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 192, 9),       # odd S: 22 nodes, the last pair full
    ([20, 20], 5, 70, 11, 3, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 512, 9),       # 36 pairs on 32 slots: second kb trip
    ([20, 20], 5, 20, 1361, 3, "mono_inv_split_k<HT=2,WM=1,EPG=16>", 512, 256),  # 11 pairs on 8 slots: second trip, idle slots
    ([64, 64, 64], 30, 20, 7, 5, "mono_inv_split_k<HT=4,WM=1,EPG=4>", 192, 9),
    ([50, 20, 33], 2, 20, 7, 5, "mono_inv_split_k<HT=4,WM=1,EPG=4>", 192, 9),    # unequal widths: padding units inert
    ([100, 100, 100], 30, 20, 7, 5, "mono_inv_split_k<HT=7,WM=1,EPG=4>", 192, 9),
    ([100, 100, 100], 30, 20, 1361, 3, "mono_inv_split_k<HT=7,WM=1,EPG=16>", 512, 256),
    ([150, 150], 30, 20, 7, 5, "mono_inv_split_k<HT=10,WM=1,EPG=4>", 192, 9),
    ([200, 200], 17, 20, 7, 5, "mono_inv_split_k<HT=16,WM=0,EPG=4>", 192, 9),    # weights from L2
    ([200], 17, 20, 7, 5, "mono_inv_split_k<HT=16,WM=1,EPG=4>", 192, 9),         # one hidden layer
    ([20] * 5, 1, 20, 7, 5, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 192, 9),        # five hidden layers, h = h0 alone
    ([20] * 7, 2, 20, 7, 5, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 192, 9),        # seven: the most the inverse accepts
    # ---- the persistent kernels: too many groups, too few nodes, or one matrix resident at a time
    ([20, 20], 5, 3, 11, 3, "mono_fwd_k<HT=2,WM=1,INV=1>", 256, 1),
    ([20, 20], 5, 8, 1639, 5, "mono_fwd_k<HT=2,WM=1,INV=1>", 256, 129),          # ngroups = 513
    ([20, 20], 5, 8, 10934, 3, "mono_fwd_k<HT=2,WM=1,INV=1>", 256, 512),         # grid capped: second grid-stride trip
    ([64, 64, 64], 30, 3, 7, 5, "mono_fwd_k<HT=4,WM=1,INV=1>", 256, 1),
    ([100, 100, 100, 100], 30, 20, 7, 5, "mono_fwd_k<HT=7,WM=2,INV=1>", 256, 1),
    ([150, 150, 150], 30, 20, 7, 5, "mono_fwd_k<HT=10,WM=2,INV=1>", 256, 1),
    ([200, 200], 17, 3, 11, 3, "mono_fwd_k<HT=16,WM=0,INV=1>", 256, 1),
    # ---- peeled nets ([49..51]^k)
    ([50, 50, 50], 30, 3, 11, 3, "mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>", 256, 1),
    ([50, 50, 50], 30, 8, 1639, 5, "mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>", 256, 129),
    ([50, 50, 50], 30, 8, 10934, 3, "mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>", 256, 512),
    ([50, 50, 50], 30, 20, 7, 5, "mono_inv_ks_x_k<HM=3,EX=2,epg=2,waves=8>", 256, 18),
    ([50, 50, 50], 30, 20, 103, 5, "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=8>", 512, 129),
    ([50, 50, 50], 30, 21, 103, 5, "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=12>", 576, 129),
    ([50, 50, 50], 30, 31, 103, 5, "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=12>", 768, 129),
    ([50, 50, 50], 30, 32, 7, 5, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=4>", 320, 9),
    ([50, 50, 50], 30, 70, 7, 5, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=4>", 576, 9),
    ([50, 50, 50], 30, 20, 1361, 3, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=16>", 704, 256),
    ([50, 50, 50], 30, 40, 1361, 3, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=16>", 768, 256),   # 21 pairs on 12 slots: two trips
    ([51, 51, 51], 30, 20, 103, 5, "mono_inv_ks_x_k<HM=3,EX=3,epg=4,waves=8>", 512, 129),
    ([51, 51, 51], 30, 20, 1361, 3, "mono_inv_split_x_k<HM=3,EX=3,WM=1,EPG=16>", 704, 256),
    ([51, 51, 51], 30, 20, 7, 5, "mono_inv_ks_x_k<HM=3,EX=3,epg=2,waves=8>", 256, 18),
    ([51, 51, 51], 30, 32, 7, 5, "mono_inv_split_x_k<HM=3,EX=3,WM=1,EPG=4>", 320, 9),
    ([51, 51, 51], 30, 3, 11, 3, "mono_fwd_x_k<HM=3,EX=3,WM=1,INV=1>", 256, 1),
    ([49, 49, 49], 30, 20, 103, 5, "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=8>", 512, 129),     # EX = 1 on the EX = 2 code
    ([49, 49, 49], 30, 20, 1361, 3, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=16>", 704, 256),
]

# Both sides of every threshold of inv_route, for the host test alone (same row format; the kernels on either side are in ROWS)
EDGES = [
    ([20, 20], 5, 6, 11, 3, "mono_fwd_k<HT=2,WM=1,INV=1>", 256, 1),                           # S < 7
    ([20, 20], 5, 7, 11, 3, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 64, 9),
    ([20, 20], 5, 20, 1360, 3, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 192, 1020),               # ngroups = 255: quarter
    ([20, 20], 5, 20, 4081, 1, "mono_inv_split_k<HT=2,WM=1,EPG=16>", 512, 256),               # ngroups = 256
    ([20, 20], 5, 20, 8192, 1, "mono_inv_split_k<HT=2,WM=1,EPG=16>", 512, 512),               # ngroups = 512
    ([20, 20], 5, 20, 8193, 1, "mono_fwd_k<HT=2,WM=1,INV=1>", 256, 129),                      # ngroups = 513
    ([50, 50, 50], 30, 20, 512, 1, "mono_inv_ks_x_k<HM=3,EX=2,epg=2,waves=8>", 256, 256),     # n <= 512: two elements
    ([50, 50, 50], 30, 20, 513, 1, "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=8>", 512, 129),
    ([50, 50, 50], 30, 31, 512, 1, "mono_inv_ks_x_k<HM=3,EX=2,epg=2,waves=8>", 384, 256),     # the most wavefronts epg = 2 takes: 6
    ([50, 50, 50], 30, 31, 4080, 1, "mono_inv_ks_x_k<HM=3,EX=2,epg=4,waves=12>", 768, 1020),  # S <= 31, ngroups = 255
    ([50, 50, 50], 30, 32, 4080, 1, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=4>", 320, 1020),
    ([50, 50, 50], 30, 31, 4081, 1, "mono_inv_split_x_k<HM=3,EX=2,WM=1,EPG=16>", 768, 256),   # not quarter: no two-step kernel
    ([50, 50, 50], 30, 6, 4081, 1, "mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>", 256, 64),
    ([50, 50, 50], 30, 20, 8193, 1, "mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>", 256, 129),
    ([50, 50, 50, 50, 50], 30, 20, 7, 5, "mono_inv_ks_x_k<HM=3,EX=2,epg=2,waves=8>", 256, 18),   # peeling is not tied to three layers
    ([50, 50, 49], 30, 20, 7, 5, "mono_inv_split_k<HT=4,WM=1,EPG=4>", 192, 9),                # ... but to equal widths
    ([52, 52, 52], 30, 20, 7, 5, "mono_inv_split_k<HT=4,WM=1,EPG=4>", 192, 9),                # H mod 16 in {1, 2, 3}
    ([48, 48, 48], 30, 20, 7, 5, "mono_inv_split_k<HT=4,WM=1,EPG=4>", 192, 9),
    ([32, 32], 5, 20, 7, 5, "mono_inv_split_k<HT=2,WM=1,EPG=4>", 192, 9),                     # pick_ht: 16 HT >= widest layer
    ([33, 20], 5, 20, 7, 5, "mono_inv_split_k<HT=4,WM=1,EPG=4>", 192, 9),
    ([65, 20], 5, 20, 7, 5, "mono_inv_split_k<HT=7,WM=1,EPG=4>", 192, 9),
    ([113, 20], 5, 20, 7, 5, "mono_inv_split_k<HT=10,WM=1,EPG=4>", 192, 9),
    ([161, 20], 5, 20, 7, 5, "mono_inv_split_k<HT=16,WM=0,EPG=4>", 192, 9),
    ([100, 100, 100], 30, 20, 8193, 1, "mono_fwd_k<HT=7,WM=1,INV=1>", 256, 129),              # image > half the LDS: one workgroup per CU
    ([100, 100, 100], 30, 8, 10934, 3, "mono_fwd_k<HT=7,WM=1,INV=1>", 256, 256),              # ... so the grid is capped at 256
]


def case_id(row):
    hidden, c, S, B, d = row[:5]
    return "%s-c%d-S%d-n%d" % ("x".join(map(str, hidden)), c, S, B * d)
