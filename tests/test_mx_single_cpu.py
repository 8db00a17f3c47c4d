"""CPU-only: the single-context form of the f16mx flat tile (csrc/tdnn_mx.hip, mx_single_kernel) ships in exactly the instantiations
mx_launch can reach, beside the twenty tdnn_mx_kernel ones that tests/test_host_cpu.py::test_library_kernel_families pins."""

import re
import subprocess

from kaldi_tflite_amd import _lib


def test_single_context_kernel_instantiations():
    out = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    single = set(re.findall(r"__device_stub__(mx_single_kernel<[^(]*>)\(", out))
    # {ReLU, none} x {planes, pooled} x {K-steps fill the super-steps, padded}: no fp32 row output on flat row tiles
    assert single == {f"mx_single_kernel<{a}, {o}, {k}>" for a in (1, 0) for o in (0, 2) for k in ("true", "false")}, single
    general = set(re.findall(r"__device_stub__(tdnn_mx_kernel<[^(]*>)\(", out))
    assert len(general) == 12 + 8, general               # the single-context form added none under that name
