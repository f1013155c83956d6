"""CPU check of the pruned last inverse butterfly of the chirp-z FFT (pta_fft.h, compiled with g++ through
tests/hostcheck/fft_pruned_check.cpp): its two outputs carry the bits of the full butterfly's outputs 0 and 1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "fft_pruned_check.cpp")
CXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off"]


@pytest.fixture(scope="module")
def fp(tmp_path_factory):
    out = tmp_path_factory.mktemp("fft_pruned") / "libfft_pruned.so"
    subprocess.check_call(CXX + ["-shared", "-fPIC", SRC, "-o", str(out)])
    return ctypes.CDLL(str(out))


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_pruned_butterfly_bit_identical_to_full(fp):
    """10^4 random butterflies after the same twiddle products (plus signed zeros, tiny and huge entries): outputs 0 and 1 of
    pta_fft_core_inv_out01<9> == those of pta_fft_core<true, 9>, compared as bit patterns."""
    rng = np.random.default_rng(64)
    n = 10000
    v = rng.standard_normal((n, 8, 2))
    v[:50] *= 1e-300
    v[50:100] *= 1e150
    v[100] = 0.0
    v[101] = -0.0
    v[102, :, 0] = 0.0
    ph = rng.uniform(0, 2 * np.pi, (n, 8))
    w = np.ascontiguousarray(np.stack([np.cos(ph), -np.sin(ph)], axis=2))
    full, pruned = np.zeros((n, 8, 2)), np.zeros((n, 2, 2))
    fp.fp_butterflies(_p(v), _p(w), n, _p(full), _p(pruned))
    assert np.all(np.isfinite(full[100:]))
    assert np.array_equal(full[:, :2].view(np.uint64), pruned.view(np.uint64))
    # and the full butterfly is the 8-point inverse DFT of the twiddled inputs (the harness feeds what it claims to)
    x = (v[200:, :, 0] + 1j * v[200:, :, 1]) * np.concatenate([np.ones((n - 200, 1)), np.conj(w[200:, 1:, 0] + 1j * w[200:, 1:, 1])], axis=1)
    ref = np.fft.ifft(x, axis=1) * 8
    got = full[200:, :, 0] + 1j * full[200:, :, 1]
    assert np.max(np.abs(got - ref)) < 1e-13 * np.max(np.abs(ref))


def test_table_twiddles_bit_identical_to_own(fp):
    """w[1], w[2], w[4] through a table + pta_fft_twiddle_products == pta_fft_twiddles<.., 1> (the shared-set path of the kernel)."""
    m = np.arange(4096)
    tw = np.stack([np.cos(2 * np.pi * m / 4096), -np.sin(2 * np.pi * m / 4096)], axis=1).ravel().copy()
    assert fp.fp_twiddle_table_mismatches(_p(tw)) == 0


def test_standalone_checker_under_sanitizers(tmp_path):
    """the same comparison as a stand-alone program with its own main(), built with AddressSanitizer + UBSan, run once"""
    exe = tmp_path / "fft_pruned_check"
    subprocess.check_call(CXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFFT_PRUNED_MAIN", SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "10000 butterflies, 0 mismatches" in r.stdout
