"""Measure the rounding allowance of the GELU regime of tests/test_gemm_forms_gpu.py on the device and write profiles/gemm_forms_gelu_error.txt.

    python tools/record_gemm_gelu_error.py [OUT]

Over the whole forward case set of the test (the small kernel's full product, the large kernel's cases, the load-form shapes) the BIAS_GELU
epilogue runs on exact z (multiples of 1/16 in [-10, 10]); per element the excess (|error| - Abramowitz-Stegun term) / max(1, |z|) against
the exact-erf fp64 reference is taken for Y = GELU(z) and G = GELU'(z), and the largest one is recorded with the z at which it occurred.
The test asserts at twice the recorded value (GELU_ROUNDING_ALLOWANCE there)."""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elegantrl_amd import ops  # noqa: E402
from tests import gemm_ref as R  # noqa: E402
from tests.test_gemm_forms_gpu import gelu_run  # noqa: E402


def main(out_path):
    dev = th.device("cuda:0")
    shapes = list(R.SMALL_FORWARD) + [c[1:4] for c in R.large_cases(R.FORWARD)] + [R.LOAD_FORM_SHAPES[R.FORWARD]]
    shapes += [s for s, _ in R.LOAD_FORM_RAGGED[R.FORWARD]]
    worst = {"Y": (-np.inf, None, None, None), "G": (-np.inf, None, None, None)}
    raw = {"Y": 0.0, "G": 0.0}
    n_z, hist = 0, np.zeros(20, np.int64)
    for shape in shapes:
        Z, Y, G = gelu_run(ops, dev, shape)
        y, gd = R.gelu_f64(Z)
        raw["Y"] = max(raw["Y"], float(np.abs(Y - y).max()))
        raw["G"] = max(raw["G"], float(np.abs(G - gd).max()))
        n_z += Z.size
        hist += np.histogram(Z, bins=20, range=(-10.0, 10.0))[0]
        for name, ex in zip(("Y", "G"), R.gelu_excess(Y, G, Z)):
            at = np.unravel_index(int(np.argmax(ex)), ex.shape)
            if ex[at] > worst[name][0]:
                worst[name] = (float(ex[at]), float(Z[at]), shape, float(np.abs((Y if name == "Y" else G)[at] - (y if name == "Y" else gd)[at])))
    allowance = max(worst["Y"][0], worst["G"][0])
    lines = [
        "Rounding allowance of the GELU regime of tests/test_gemm_forms_gpu.py (tools/record_gemm_gelu_error.py), measured on " +
        f"{th.cuda.get_device_name(0)} ({th.cuda.get_device_properties(0).gcnArchName}).",
        "BIAS_GELU epilogue of csrc/gemm_tiles.h (gelu_and_grad_fast) on exact z, multiples of 1/16 in [-10, 10], against exact-erf GELU and",
        "Phi(z) + z phi(z) in fp64.  excess = (|error| - A&S term) / max(1, |z|); A&S term: 0.75e-7 |z| for Y, 0.75e-7 for G.",
        "",
        f"forward shapes: {len(shapes)}    z values checked: {n_z}    z per unit interval of [-10, 10]: {hist.tolist()}",
        f"largest |Y - GELU(z)|:  {raw['Y']:.4e}        largest |G - GELU'(z)|: {raw['G']:.4e}",
    ]
    for name in ("Y", "G"):
        ex, z, shape, err = worst[name]
        lines.append(f"largest excess of {name}: {ex:.4e} at z = {z} (|error| {err:.4e}), shape (rows, Nw, K) = {shape}")
    lines += ["", f"allowance (the larger of the two): {allowance:.4e}",
              f"asserted rounding part of the bar: 2 x allowance = {2 * allowance:.4e} x max(1, |z|)   (must stay below 1e-6)"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gemm_forms_gelu_error.txt"))
