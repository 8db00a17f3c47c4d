#!/usr/bin/env python3
"""
Golden-vector generator for dense PLDA scoring with conversation-dependent PCA (test infrastructure; runs only in the
build container, next to make_golden.py).

Reads the reference's Kaldi-generated table of `ivector-plda-scoring-dense` scores WITH the per-recording PCA
(testdata/plda/plda_scores.py, RefPldaScores.ark: the 29 x-vectors of plda.npz scored as one recording) and writes
tests/golden/plda_dense.npz. Its inputs are already committed: plda.npz["plda_input"] and plda.bin. DATA only.

Usage:  python tests/golden/make_golden_dense.py
"""

import importlib.util
import os

import numpy as np

REF = "/root/reference"
TD = os.path.join(REF, "kaldi_tflite/lib/testdata")
OUT = os.path.dirname(os.path.abspath(__file__))
TARGET_ENERGY = 0.1     # the table's --target-energy (a restatement reproduces it at 0.1 only)


def load_py(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sc = load_py(os.path.join(TD, "plda/plda_scores.py"), "ref_plda_scores").RefPldaScores
    scores = np.asarray(sc.scores(withoutPCA=False))
    assert scores.shape == (29, 29), scores.shape
    np.savez_compressed(os.path.join(OUT, "plda_dense.npz"), plda_dense_scores=scores,
                        target_energy=np.float64(TARGET_ENERGY),
                        provenance=np.array("kaldi_tflite/lib/testdata/plda/plda_scores.py RefPldaScores.ark: Kaldi "
                                            "ivector-plda-scoring-dense --target-energy 0.1 on the 29 vectors of "
                                            "plda.npz['plda_input'] (one recording) with the model plda.bin"))
    print("wrote plda_dense.npz", scores.shape, scores.dtype)


if __name__ == "__main__":
    main()
