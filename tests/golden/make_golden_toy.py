"""The law of the reference's toy problems, from the REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_toy.py      # writes tests/golden/toy_law.npz

Loads the reference's lib/toy_data.py by path (it needs numpy, torch, scikit-learn and PIL, nothing of the reference's models)
and reduces samples of `inf_train_gen` to statistics -- data only, no sample is stored:

  * for each of the fourteen base problems (tests/toy_ref.py: KINDS), N_DRAWS = 8 independent draws of N_LAW = 65 536 samples
    (pinwheel: 65 535, it returns 5 (B // 5) rows): the 32 x 32 histogram over [-6, 6]^2 with samples clipped (`hist`, int32
    [14, 8, 32, 32]), the mean vector (`mean` [14, 8, 2]) and the covariance entries xx, xy, yy (`cov` [14, 8, 3]).  Draw k is
    seeded with np.random.RandomState(k) for the generator that is handed in, and np.random.seed(GLOBAL_SEED + k) /
    torch.manual_seed(GLOBAL_SEED + k) for checkerboard, cos, joint_gaussian and scikit-learn's generators, which use the global
    ones.  (Not seed k for both: RandomState(k) and np.random.seed(k) are the SAME Mersenne-Twister stream, so `cos` would
    take its abscissa and its noise, and 8-MIX its 2spirals and swissroll blocks, from the same numbers -- a correlation of
    0.41 between columns 0 and 4 of 8-MIX that the reference's law does not have);
  * one 8-MIX batch of B_MIX = 16 390 rows (its pinwheel block needs a multiple of 5, its 2spirals block an even number: the
    reference raises on any other batch), the first N_MIX = 16 384 kept: mean and standard deviation per column (`mix_mean`,
    `mix_std` [16]) and the correlation matrix (`mix_corr` [16, 16])."""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toy_ref  # noqa: E402

from make_golden import OUT, REF  # noqa: E402  (where the reference lies, and this directory)

REF_TOY_DATA = os.path.join(REF, "lib", "toy_data.py")
GLOBAL_SEED = 1000


def _load():
    spec = importlib.util.spec_from_file_location("reference_toy_data", REF_TOY_DATA)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _draw(mod, name, n, k):
    np.random.seed(GLOBAL_SEED + k)
    torch.manual_seed(GLOBAL_SEED + k)
    x = mod.inf_train_gen(name, rng=np.random.RandomState(k), batch_size=n)
    return np.asarray(x, dtype=np.float64)


def main():
    mod = _load()
    nk = len(toy_ref.KINDS)
    hist = np.zeros((nk, toy_ref.N_DRAWS, toy_ref.BINS, toy_ref.BINS), dtype=np.int32)
    mean = np.zeros((nk, toy_ref.N_DRAWS, 2))
    cov = np.zeros((nk, toy_ref.N_DRAWS, 3))
    for i, name in enumerate(toy_ref.KINDS):
        n = toy_ref.N_LAW - 1 if name == "pinwheel" else toy_ref.N_LAW
        for k in range(toy_ref.N_DRAWS):
            x = _draw(mod, name, n, k)
            assert x.shape == (n, 2), (name, x.shape)
            hist[i, k] = toy_ref.histogram(x)
            mean[i, k], cov[i, k] = toy_ref.moments(x)
        print(name, "mean", mean[i].mean(0), "cov", cov[i].mean(0), flush=True)
    mix = _draw(mod, "8-MIX", toy_ref.B_MIX, 0)[:toy_ref.N_MIX]
    assert mix.shape == (toy_ref.N_MIX, 16)
    mix_mean, mix_std, mix_corr = toy_ref.mix_stats(mix)
    path = os.path.join(OUT, "toy_law.npz")
    np.savez_compressed(path, names=np.array(toy_ref.KINDS), hist=hist, mean=mean, cov=cov, mix_mean=mix_mean,
                        mix_std=mix_std, mix_corr=mix_corr)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
