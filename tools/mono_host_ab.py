#!/usr/bin/env python
"""A/B of the Monotonic unit's host half: what one build of libgnf_hip.so answers and computes, as text that two builds'
runs can be diffed on (profiles/mono_host_ab.txt).  One process per build; the library is loaded by path.

    python tools/mono_host_ab.py --host LIB               # CPU: pack_floats and bwd_ws_bytes over a grid of nets -> stdout
    python tools/mono_host_ab.py --gpu LIB --out FILE     # one line per output tensor: case, entry, tensor, sha256, reporter
                                [--only fwd,inv,bwd | inv-peeled | bwd-narrow]

GNF_MONO_INDW / GNF_MONO_INV_PTS are read once per process by the library: set them in the environment of the run
(--only inv-peeled and bwd-narrow are the case subsets those switches can move)."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")]

import torch  # noqa: E402  (the HIP runtime first, then the library)
from gnf_hip import abi  # noqa: E402

MIXED = [[40, 64, 24], [97, 110, 101], [145, 158, 147], [100, 150, 100], [48, 50, 50, 50]]   # test_monotonic_forward_backward_vs_oracle
HS = [1, 10, 16, 17, 32, 33, 48, 49, 50, 51, 52, 64, 65, 97, 100, 112, 113, 145, 150, 160, 161, 200, 256, 257]
CS = [1, 5, 30, 32, 33, 63, 600]
SBD = [(20, 1, 1), (20, 100, 784), (150, 50000, 63), (9, 0, 5), (250, 50, 63)]


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in abi.SIGNATURES.items():
        if name.startswith("gnf_monotonic") or name == "gnf_gemm_split_enabled":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def host(lib):
    for hidden in [[H] * NH for H in HS for NH in range(1, 6)] + MIXED:
        for c in CS:
            net = abi.MonoNet()
            net.nl = len(hidden) + 1
            for i, v in enumerate([1 + c] + hidden + [1]):
                net.dims[i] = v
            ws = [lib.gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d) for S, B, d in SBD]
            print(hidden, c, lib.gnf_monotonic_pack_floats(ctypes.byref(net)), *ws)


# ---------------------------------------------------------------------------------------------------------------- GPU cases
# forward: (hidden, c) at two sizes (B, d, S).  Route each case reaches (profiles/mono_host_ab.txt lists them again):
FWD = [([100] * 3, 30), ([150, 150], 5), ([150] * 4, 30),                    # wide
       ([50] * 3, 30), ([49, 49], 8), ([51] * 3, 30), ([50], 30),            # peeled split / fp32; NH = 1: no split
       ([51] * 4, 30),                                                       # peeled, split does not fit half the LDS
       ([50], 600),                                                          # peeled, image not resident
       ([10], 5), ([40, 64, 24], 5), ([100], 5), ([150], 5),                 # by HT, image resident
       ([150] * 3, 33), ([112] * 4, 33), ([50] * 3, 600),                    # one matrix at a time
       ([200, 200], 8)]                                                      # streamed
FWD_SIZES = [(40, 13, 20), (7, 3, 9)]
# inverse: (hidden, c, n, S), d = 1; both entries
PEELED_INV = ([([H] * 3, 30, n, S) for n, S, H in
               [(700, 20, 50), (37, 20, 50), (3, 27, 50), (1000, 30, 50), (700, 7, 50), (512, 20, 50), (513, 20, 50), (301, 31, 50),
                (100, 40, 50), (300, 32, 50), (700, 20, 51), (200, 20, 51), (700, 20, 49), (64, 9, 49)]] +   # tests/test_gpu_parity.py
              [([50] * 3, 30, 5000, 20), ([50] * 3, 30, 9000, 20), ([50] * 3, 30, 700, 5),
               ([50], 600, 63, 20), ([50], 600, 700, 20), ([50], 600, 5000, 20), ([50], 600, 9000, 20)])   # image not resident
INV = PEELED_INV + [([100] * 3, 30, 63, 20), ([100] * 3, 30, 5000, 20), ([16, 16], 5, 63, 20), ([16, 16], 5, 5000, 20),
                    ([16, 16], 5, 9000, 20), ([16, 16], 5, 63, 5), ([200, 200], 8, 63, 20), ([200, 200], 8, 5000, 20),
                    ([200, 200], 8, 9000, 20), ([150] * 3, 33, 63, 20), ([150] * 3, 33, 9000, 20)]
# backward: (hidden, c) at (B, d, S) = (5, 8, 20) [also with the one-chunk workspace] and (40, 13, 21)
NARROW_BWD = [([50] * 3, 30), ([20, 20], 5), ([48, 50, 50, 50], 5), ([40, 64, 24], 5), ([51] * 3, 30), ([49, 49], 8), ([10], 5),
              ([50] * 4, 30), ([64, 64], 5), ([50], 30)]
BWD = NARROW_BWD + [([150] * 3, 30), ([100, 100], 33), ([200, 200], 8), ([100], 5), ([100] * 4, 30), ([112] * 4, 30), ([150] * 4, 30),
                    ([150, 150], 5), ([150] * 3, 33), ([97, 110, 101], 30), ([100] * 3, 30)]
BWD_SIZES = [(5, 8, 20), (40, 13, 21)]


class Run:
    def __init__(self, lib, out):
        self.lib, self.out, self.dev = lib, out, "cuda:0"

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s -> %d" % (what, rc))

    def params(self, hidden, c, seed):
        g = torch.Generator().manual_seed(seed)
        dims = [1 + c] + list(hidden) + [1]
        ps = []
        for i in range(len(dims) - 1):
            bound = 1.3 / dims[i] ** .5
            ps.append(((torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bound * 1.7).to(self.dev))
            ps.append(((torch.rand(dims[i + 1], generator=g) * 2 - 1) * bound).to(self.dev))
        return ps

    def net_pack(self, params):
        from gnf_hip import ops
        net = ops._mono_net(params)
        nfl = self.lib.gnf_monotonic_pack_floats(ctypes.byref(net))
        pack = torch.empty(int(nfl), device=self.dev)
        self.check(self.lib.gnf_monotonic_pack(ctypes.byref(net), abi.ptr(pack), self.stream()), "pack")
        return net, pack

    def emit(self, case, entry, tensors):
        torch.cuda.synchronize()
        rep = "%s|%s" % (self.lib.gnf_monotonic_fwd_kernel().decode(), self.lib.gnf_monotonic_bwd_kernel().decode())
        for name, t in tensors:
            digest = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            self.out.write("%s %s %s %s %s\n" % (case, entry, name, digest, rep))
        self.out.flush()

    def data(self, B, d, c, seed):
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn(B, d, generator=g) * 2.).to(self.dev)
        h = torch.randn(B, d, c, generator=g).to(self.dev)
        return x, h, torch.randn(B, d, generator=g).to(self.dev), torch.randn(B, d, generator=g).to(self.dev)

    def fwd(self, hidden, c, B, d, S):
        from gnf_hip import ops
        ptr = abi.ptr
        net, pack = self.net_pack(self.params(hidden, c, sum(hidden) + c))
        x, h, _, _ = self.data(B, d, c, B + d)
        w, t = ops.cc_rule(S, self.dev)
        case = "fwd:%s:c%d:B%d:d%d:S%d" % ("-".join(map(str, hidden)), c, B, d, S)
        for entry in ("gnf_monotonic_fwd", "gnf_monotonic_fwd_f32"):
            z, jac = torch.zeros_like(x), torch.zeros_like(x)
            self.check(getattr(self.lib, entry)(ptr(pack), ctypes.byref(net), ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2),
                                                ptr(w), ptr(t), S, ptr(z), ptr(jac), B, d, self.stream()), entry)
            self.emit(case, entry, [("z", z), ("jac", jac)])

    def inv(self, hidden, c, n, S):
        from gnf_hip import ops
        ptr = abi.ptr
        net, pack = self.net_pack(self.params(hidden, c, sum(hidden) + c + 1))
        z, h, _, _ = self.data(n, 1, c, n + S)
        z = z * 1.5
        w, t = ops.cc_rule(S, self.dev)
        case = "inv:%s:c%d:n%d:S%d" % ("-".join(map(str, hidden)), c, n, S)
        x = torch.zeros_like(z)
        self.check(self.lib.gnf_monotonic_inv(ptr(pack), ctypes.byref(net), ptr(z), ptr(h), h.stride(0), h.stride(1), h.stride(2),
                                              ptr(w), ptr(t), S, ptr(x), n, 1, self.stream()), "inv")
        self.emit(case, "gnf_monotonic_inv", [("x", x)])
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(torch.int32).to(self.dev)
        x = torch.zeros_like(z)
        self.check(self.lib.gnf_monotonic_inv_scatter(ptr(pack), ctypes.byref(net), ptr(z), ptr(h), h.stride(0), h.stride(1),
                                                      h.stride(2), ptr(w), ptr(t), S, ptr(x), ctypes.c_void_p(rows.data_ptr()), 1,
                                                      n, 1, self.stream()), "inv_scatter")
        self.emit(case, "gnf_monotonic_inv_scatter", [("x", x)])

    def bwd(self, hidden, c, B, d, S, chunked):
        from gnf_hip import ops
        ptr = abi.ptr
        params = self.params(hidden, c, sum(hidden) + c + 2)
        net, pack = self.net_pack(params)
        x, h, gz, gjac = self.data(B, d, c, B + d + 1)
        w, t = ops.cc_rule(S, self.dev)
        case = "bwd:%s:c%d:B%d:d%d:S%d" % ("-".join(map(str, hidden)), c, B, d, S)
        full = self.lib.gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d)
        runs = [("gnf_monotonic_bwd", full, ""), ("gnf_monotonic_bwd_f32", full, "")]
        if chunked:
            one = self.lib.gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, 1, 1)
            runs += [("gnf_monotonic_bwd", one, "/chunked"), ("gnf_monotonic_bwd_f32", one, "/chunked")]
        nl = net.nl
        for entry, nbytes, tag in runs:
            gx, gh = torch.zeros_like(x), torch.zeros_like(h)
            gp = [torch.zeros_like(p) for p in params]
            gW = (ctypes.c_void_p * nl)(*[gp[2 * l].data_ptr() for l in range(nl)])
            gb = (ctypes.c_void_p * nl)(*[gp[2 * l + 1].data_ptr() for l in range(nl)])
            ws = torch.zeros(max(nbytes // 4, 1), device=self.dev)
            self.check(getattr(self.lib, entry)(ptr(pack), ctypes.byref(net), ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2),
                                                ptr(w), ptr(t), S, ptr(gz), ptr(gjac), ptr(gx), ptr(gh), gh.stride(0), gh.stride(1),
                                                gh.stride(2), gW, gb, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, B, d,
                                                self.stream()), entry)
            self.emit(case, entry + tag, [("gx", gx), ("gh", gh)] + [("gp%d" % i, p) for i, p in enumerate(gp)])


def gpu(lib, out, only):
    r = Run(lib, out)
    if "fwd" in only:
        for hidden, c in FWD:
            for B, d, S in FWD_SIZES:
                r.fwd(hidden, c, B, d, S)
    if "inv" in only or "inv-peeled" in only:
        for hidden, c, n, S in (INV if "inv" in only else PEELED_INV):
            r.inv(hidden, c, n, S)
    if "bwd" in only or "bwd-narrow" in only:
        for hidden, c in (BWD if "bwd" in only else NARROW_BWD):
            for k, (B, d, S) in enumerate(BWD_SIZES):
                r.bwd(hidden, c, B, d, S, chunked=k == 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", metavar="LIB")
    ap.add_argument("--gpu", metavar="LIB")
    ap.add_argument("--out")
    ap.add_argument("--only", default="fwd,inv,bwd")
    a = ap.parse_args()
    if a.host:
        host(load(a.host))
    if a.gpu:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            gpu(load(a.gpu), f, a.only.split(","))


if __name__ == "__main__":
    main()
