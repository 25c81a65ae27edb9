"""Generator of tests/golden/frechet_small.npz: the REFERENCE's `calculate_frechet_distance`
(sgam/generative_sensing_module/modules/misc/pytorch_fid/fid_score.py) on seeded (mu, sigma) pairs.  Build-container only, like
gen_golden.py: it imports the reference's file and writes arrays and recorded results, nothing else.

    python tests/golden/gen_golden_fid.py

fid_score.py and the inception.py next to it import torchvision, which is not installed: the stubs below stand in for it (the
three Inception block classes are only subclassed at import time; nothing of them runs).  The two files are loaded as a package
of their own, so none of the reference's other modules is imported.

Cases: d = 8 and d = 64, each with N = 200 samples per side (full rank) and N = 40 (for d = 64 the covariances have rank 39:
the singular product the function repairs with its eps retry).  `retried` records whether the retry message was printed."""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402  (only for where the reference lives: its install() stubs are not used here)

REF_FID = os.path.join(R.REF, "sgam", "generative_sensing_module", "modules", "misc", "pytorch_fid")

if not os.path.isfile(os.path.join(REF_FID, "fid_score.py")):
    raise SystemExit("the reference is not available: fixtures can only be generated where it is")


def install_stubs():
    tv = types.ModuleType("torchvision")
    tv.__version__ = "0.0"
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.inception = types.ModuleType("torchvision.models.inception")
    for name in ("InceptionA", "InceptionC", "InceptionE"):
        setattr(tv.models.inception, name, type(name, (nn.Module,), {}))
    for m in (tv, tv.transforms, tv.models, tv.models.inception):
        sys.modules[m.__name__] = m
    pkg = types.ModuleType("ref_pytorch_fid")
    pkg.__path__ = [REF_FID]
    sys.modules["ref_pytorch_fid"] = pkg


def sample_statistics(rng, n, d, shift):
    mix = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    act = rng.standard_normal((n, d)) @ mix + shift * rng.standard_normal(d)
    return act.mean(axis=0), np.cov(act, rowvar=False)


def main():
    install_stubs()
    ref = importlib.import_module("ref_pytorch_fid.fid_score")
    out = {}
    names = []
    for d in (8, 64):
        for n in (200, 40):
            rng = np.random.default_rng(1000 * d + n)
            mu1, s1 = sample_statistics(rng, n, d, 0.5)
            mu2, s2 = sample_statistics(rng, n, d, 0.7)
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                value = ref.calculate_frechet_distance(mu1, s1, mu2, s2)
            name = f"d{d}_n{n}"
            names.append(name)
            out.update({f"{name}_mu1": mu1, f"{name}_sigma1": s1, f"{name}_mu2": mu2, f"{name}_sigma2": s2,
                        f"{name}_fid": np.float64(value), f"{name}_retried": np.bool_("singular" in said.getvalue())})
            print(name, float(value), "retried" if "singular" in said.getvalue() else "")
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "frechet_small.npz"), **out)


if __name__ == "__main__":
    main()
