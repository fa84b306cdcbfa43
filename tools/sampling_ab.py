#!/usr/bin/env python
"""A/B of the sampling paths of NormalizingFlowStep / FCNormalizingFlow: what one checkout computes through invert, intervene,
counterfactual, rsample (and its backward), forward_do / log_prob_do / loss_do and loss, as text that the runs of two
checkouts can be diffed on (profiles/sampling_refactor_ab.txt).  One process per checkout; the package is imported from --root.

    python tools/sampling_ab.py --root DIR --out FILE [--detail]

--detail: one line per case and batch size (0, 1, 17): per call, the first 12 hex digits of one sha256 over every tensor it returned
(rsample: x and the gradients of z, the context and every parameter) with `_intervene_arm` / `_rsample_arm`, and the kinds of the
step's `_INV_GRAPHS` entries (warm / eager / captured); a call that raises is recorded with its exception's class and a digest
of its text.  Without it, one line per case: one sha256 over those detailed lines and, per batch size, the arms of the intervene calls
run-length coded by first letter (None / levels / columns / passes), rsample's arm and the graph kinds -- the form that is
committed; --detail finds the call behind a difference.
Then one line per argument error of do_arguments / do_targets and per refusal, with its text.  Fixed seeds, no timing."""
import argparse
import hashlib
import itertools
import os
import sys

DEV = "cuda:0"
DETAIL = False            # --detail: every call's digest instead of one per line
BATCHES = (0, 1, 17)


def digest(out):
    """the first 12 hex digits of ONE sha256 over every tensor a call returned, in order (None and non-tensors by their repr)"""
    import torch
    h = hashlib.sha256()
    for t in (out if isinstance(out, (tuple, list)) else (out,)):
        h.update(t.detach().contiguous().cpu().numpy().tobytes() if torch.is_tensor(t) else repr(t).encode())
        h.update(b"|")
    return h.hexdigest()[:12]


def guard(fn, full=False):
    """the digest of fn()'s tensors, or the exception it raises -- its class and a digest of its text, or the text itself
    with full=True: both trees must agree on either"""
    try:
        return digest(fn())
    except Exception as exc:                            # noqa: BLE001
        text = " ".join(str(exc).split())
        return "%s(%s)" % (type(exc).__name__, text if full else hashlib.sha256(text.encode()).hexdigest()[:8])


def normalizer(norm):
    import models
    return {"affine": (models.AffineNormalizer, {}, 2),
            "spline": (models.SplineNormalizer, {"nb_bins": 4, "tail_bound": 3.}, 11),
            "mono": (models.MonotonicNormalizer, {"integrand_net": [8, 8], "cond_size": 4, "nb_steps": 8, "solver": "CC"}, 4)}[norm]


def flow_of(kind, d, c, hidden, norm, seed, graph="chain", hot=True, frozen=True):
    import torch
    import models
    N, nkw, out = normalizer(norm)
    torch.manual_seed(seed)
    cond = {"made": models.AutoregressiveConditioner, "dag": models.DAGConditioner, "coupling": models.CouplingConditioner}[kind]
    kw = {"in_size": d, "hidden": list(hidden), "out_size": out, "cond_in": c}
    if kind == "dag":
        kw["hot_encoding"] = hot
    flow = models.buildFCNormalizingFlow(1, cond, kw, N, nkw)
    if kind == "dag":
        cnd = flow.steps[0].conditioner
        A = torch.zeros(d, d)
        if graph == "chain":
            A[torch.arange(1, d), torch.arange(d - 1)] = 1.
        else:                                           # a random DAG at density .3 in a random topological order
            gen = torch.Generator().manual_seed(d)
            perm = torch.randperm(d, generator=gen)
            A[perm[:, None], perm[None, :]] = torch.tril((torch.rand(d, d, generator=gen) < .3).float(), -1)
        with torch.no_grad():
            cnd.A.copy_(A)
        cnd.stoch_gate = cnd.noise_gate = cnd.s_thresh = False
        cnd.h_thresh = 0.
        cnd.A.requires_grad = not frozen
        cnd.invalidate_caches()
    return flow.to(DEV)


def pin_sets(d):
    sets = [[], [0], [t for t in (d // 2 - 1, d // 2) if 0 <= t < d], list(range(0, d, 2)), list(range(d))]
    return [s for k, s in enumerate(sets) if s not in sets[:k]]


def run_case(name, flow, d, c, emit, switches=()):
    import torch
    from models.NormalizingFlow import _INV_GRAPHS
    step = flow.steps[0]
    for flag in switches:
        setattr(step, flag, False)
    brief = []
    for B in BATCHES:
        gen = torch.Generator().manual_seed(1000 * d + 10 * c + B)
        z = (.7 * torch.randn(B, d, generator=gen)).to(DEV)
        ctx = torch.randn(B, c, generator=gen).to(DEV) if c else None
        v = torch.randn(B, d, generator=gen).to(DEV)
        vs = torch.randn(d, generator=gen).to(DEV)
        cot = torch.randn(B, d, generator=gen).to(DEV)
        out = []
        out.append("invert=" + "/".join(guard(lambda: step.invert(z, ctx)) for _ in range(3)))
        for idx in pin_sets(d):
            for what, vals in (("s", .25), ("S", vs[idx]), ("BS", v[:, idx])):
                step._intervene_arm = "unset"
                out.append("do%s%s=%s:%s" % (len(idx), what, guard(lambda: step.intervene(z, idx, vals, ctx)), step._intervene_arm))
        out.append("do_tensor=" + guard(lambda: step.intervene(z, torch.tensor(pin_sets(d)[1]), v[:, pin_sets(d)[1]], ctx)))
        out.append("cf=" + guard(lambda: flow.counterfactual(v, pin_sets(d)[1], .5, ctx)))

        def rsample():
            zz = z.clone().requires_grad_(True)
            cc = None if ctx is None else ctx.clone().requires_grad_(True)
            for p in flow.parameters():
                p.grad = None
            x = flow.rsample(zz, cc)
            x.backward(cot)
            return [x, zz.grad, None if cc is None else cc.grad] + [p.grad for p in flow.parameters()]
        step._rsample_arm = "unset"
        out.append("rsample=%s:%s" % (guard(rsample), step._rsample_arm))
        mask = torch.zeros(d, dtype=torch.bool)
        mask[::2] = True
        table = torch.zeros(3, d, dtype=torch.uint8)
        table[1, 0] = 1
        table[2, d - 1:] = 1
        regime = (torch.arange(B) % 3).to(DEV)
        for what, targets, reg in (("idx", sorted({0, d - 1}), None), ("mask", mask.to(DEV), None),
                                   ("table", table.to(DEV), regime), ("empty", [], None)):
            out.append("fdo_%s=%s" % (what, guard(lambda: step.forward_do(v, targets, reg, ctx))))
            out.append("lpdo_%s=%s" % (what, guard(lambda: flow.log_prob_do(v, targets, reg, ctx))))
            out.append("ldo_%s=%s" % (what, guard(lambda: flow.loss_do(v, targets, reg, ctx))))
        out.append("loss=" + guard(lambda: flow.loss(*flow(v, ctx))))
        kinds = sorted("captured" if isinstance(e, tuple) else str(e) for e in _INV_GRAPHS.get(step, {}).values())
        out.append("graphs=" + ("+".join(kinds) or "none"))
        if DETAIL:
            emit("%s B=%d %s" % (name, B, " ".join(out)))
        arms = "".join(f.rsplit(":", 1)[1][0] for f in out if f.startswith("do") and ":" in f)
        brief.append((" ".join(out), "x".join("%s%d" % (a, len(list(g))) for a, g in itertools.groupby(arms)),
                      str(step._rsample_arm).replace(" ", ""), out[-1][7:]))
    if not DETAIL:
        # one digest over the lines --detail prints, beside what reads as text, per batch size: the arms of the intervene
        # calls run-length coded by their first letters, rsample's arm, the graph kinds
        emit("%s %s arms=%s rsample=%s graphs=%s" % ((name, hashlib.sha256("\n".join(b[0] for b in brief).encode()).hexdigest()[:16])
                                                     + tuple("/".join(b[k] for b in brief) for k in (1, 2, 3))))


def sampling(emit):
    for hidden in ([], [16], [40, 33, 19]):
        for d in (1, 6, 17):
            for c in (0, 2):
                for norm in ("affine", "spline", "mono"):
                    name = "made %s h=%s d=%d c=%d" % (norm, "x".join(map(str, hidden)) or "none", d, c)
                    run_case(name, flow_of("made", d, c, hidden, norm, seed=d + c), d, c, emit)
    for graph in ("chain", "random"):
        for d in (6, 43):
            for c, hot in ((0, True), (0, False), (2, True)):       # (without the one-hot: the pass of c = 0 is captured)
                for norm in ("affine", "spline"):
                    name = "dag %s %s d=%d c=%d hot=%d" % (graph, norm, d, c, hot)
                    run_case(name, flow_of("dag", d, c, [16], norm, seed=d + c, graph=graph, hot=hot), d, c, emit)
    run_case("dag chain affine d=6 c=0 trainable A", flow_of("dag", 6, 0, [16], "affine", 3, frozen=False), 6, 0, emit)
    flow = flow_of("dag", 6, 0, [16], "affine", 4, graph="random")
    flow.steps[0].conditioner.h_thresh = .5
    run_case("dag random affine d=6 c=0 h_thresh=.5", flow, 6, 0, emit)
    for c in (0, 2):
        run_case("coupling affine d=6 c=%d" % c, flow_of("coupling", 6, c, [16], "affine", 5), 6, c, emit)
    off = ("column_schedule", "level_schedule")
    run_case("made mono h=16 d=6 c=2 fast arms off", flow_of("made", 6, 2, [16], "mono", 6), 6, 2, emit, off)
    run_case("dag chain spline d=6 c=2 fast arms off", flow_of("dag", 6, 2, [16], "spline", 7), 6, 2, emit, off)


def refusals(emit):
    import torch
    from models.NormalizingFlow import do_arguments, do_targets
    z = torch.zeros(4, 5)
    i64 = lambda *a: torch.tensor(a, dtype=torch.int64)
    errors = {
        "args z rank": lambda: do_arguments([0], 0., torch.zeros(5)),
        "args float tensor": lambda: do_arguments(torch.tensor([0.]), 0., z),
        "args bool tensor": lambda: do_arguments(torch.tensor([True]), 0., z),
        "args 2-d tensor": lambda: do_arguments(i64(0, 1).view(1, 2), 0., z),
        "args uint8 tensor is an index list": lambda: do_arguments(torch.tensor([1, 3], dtype=torch.uint8), 0., z)[0],
        "args float element": lambda: do_arguments([0, 1.], 0., z),
        "args bool element": lambda: do_arguments([0, True], 0., z),
        "args not iterable": lambda: do_arguments(3, 0., z),
        "args range": lambda: do_arguments([0, 5], 0., z),
        "args negative": lambda: do_arguments(i64(-1), 0., z),
        "args twice": lambda: do_arguments([2, 2], 0., z),
        "args value shape": lambda: do_arguments([0, 1], torch.zeros(3), z),
        "args value type": lambda: do_arguments([0, 1], "v", z),
        "targets x rank": lambda: do_targets([0], None, torch.zeros(5)),
        "targets mask width": lambda: do_targets(torch.zeros(4, dtype=torch.bool), None, z),
        "targets mask rank": lambda: do_targets(torch.zeros(1, 1, 5, dtype=torch.bool), None, z),
        "targets mask rows": lambda: do_targets(torch.zeros(3, 5, dtype=torch.uint8), None, z),
        "targets regime with [d] mask": lambda: do_targets(torch.zeros(5, dtype=torch.bool), i64(0, 0, 0, 0), z),
        "targets regime with indices": lambda: do_targets([0], i64(0, 0, 0, 0), z),
        "targets float tensor": lambda: do_targets(torch.tensor([0.]), None, z),
        "targets 2-d tensor": lambda: do_targets(i64(0, 1).view(1, 2), None, z),
        "targets uint8 tensor is a mask": lambda: do_targets(torch.tensor([1, 3], dtype=torch.uint8), None, z),
        "targets not iterable": lambda: do_targets(3, None, z),
        "targets float element": lambda: do_targets([0, 1.], None, z),
        "targets bool element": lambda: do_targets([0, True], None, z),
        "targets range": lambda: do_targets([0, 5], None, z),
        "targets twice": lambda: do_targets([2, 2], None, z),
        "targets regime dtype": lambda: do_targets(torch.zeros(2, 5, dtype=torch.bool), torch.zeros(4), z),
        "targets regime length": lambda: do_targets(torch.zeros(2, 5, dtype=torch.bool), i64(0, 1), z),
        "targets regime not a tensor": lambda: do_targets(torch.zeros(2, 5, dtype=torch.bool), [0, 1, 0, 1], z),
        "targets regime ids": lambda: do_targets(torch.zeros(2, 5, dtype=torch.bool), i64(0, 1, 2, 0), z),
    }
    for name, fn in errors.items():
        emit("error %s: %s" % (name, guard(fn, full=True)))
    flow = flow_of("dag", 6, 0, [16], "affine", 8)
    cond = flow.steps[0].conditioner
    cond.stoch_gate, cond.s_thresh = True, True
    zz = torch.zeros(3, 6, device=DEV)
    for name, fn in (("intervene", lambda: flow.intervene(zz, [0], 0.)), ("counterfactual", lambda: flow.counterfactual(zz, [0], 0.)),
                     ("rsample", lambda: flow.rsample(zz)), ("step.intervene", lambda: flow.steps[0].intervene(zz, [0], 0.))):
        emit("refusal %s: %s" % (name, guard(fn, full=True)))
    two = flow_of("made", 6, 0, [16], "affine", 9)
    two.steps.append(flow_of("made", 6, 0, [16], "affine", 10).steps[0])
    for name, fn in (("intervene", lambda: two.intervene(zz, [0], 0.)), ("log_prob_do", lambda: two.log_prob_do(zz, [0])),
                     ("invert", lambda: two.invert(zz)), ("rsample", lambda: two.rsample(zz))):
        emit("two steps %s: %s" % (name, guard(fn, full=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the checkout (built) whose package is imported")
    ap.add_argument("--out", default=None)
    ap.add_argument("--detail", action="store_true")
    args = ap.parse_args()
    global DETAIL
    DETAIL = args.detail
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "graphical-normalizing-flows_amd")]
    import torch
    import models
    assert os.path.abspath(models.__file__).startswith(root + os.sep), models.__file__
    assert torch.cuda.is_available(), "the cases run on the MI355X"
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    sampling(emit)
    refusals(emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
