"""Philox4x32-10 (egc_amd/csrc/egc_philox.h), run on the host by tests/philox/philox_check.cpp: the three known answers of
Random123's kat_vectors, and 1,000 random counters and keys word for word against the numpy function of tests/gat_dropout_ref.py
(which the attention-dropout tests build their masks from)."""
import os
import subprocess

import numpy as np
import pytest

from gat_dropout_ref import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "philox", "_build", "philox_check")

KNOWN = (
    ("00000000 00000000 00000000 00000000 00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344 a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


@pytest.fixture(scope="module")
def program():
    subprocess.run(["bash", os.path.join(ROOT, "tests", "philox", "build.sh")], check=True, capture_output=True)

    def run(rows):
        """[n, 4] uint32 words for [n, 6] uint32 inputs (counter, key)."""
        text = "".join(" ".join(f"{int(v):08x}" for v in row) + "\n" for row in rows)
        r = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [line for line in r.stdout.split("\n") if line]
        assert len(lines) == len(rows)
        return np.array([[int(w, 16) for w in line.split()] for line in lines], dtype=np.uint32)
    return run


def _parse(text):
    return [int(w, 16) for w in text.split()]


def test_known_answers(program):
    got = program([_parse(inp) for inp, _ in KNOWN])
    for (inp, want), row in zip(KNOWN, got):
        assert [int(v) for v in row] == _parse(want), inp
        v = np.array(_parse(inp), dtype=np.uint64)
        assert [int(w) for w in philox4x32_10(v[:4], v[4:])] == _parse(want), inp       # and the numpy function


def test_a_thousand_random_counters_and_keys_match_numpy(program):
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 2 ** 32, size=(1000, 6), dtype=np.uint64)
    rows[:8, 0] = np.arange(8)                       # small counters, as the kernels use them
    rows[:8, 1:4] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 1, 0]] * 2
    got = program(rows)
    want = philox4x32_10(rows[:, :4], rows[:, 4:])
    assert got.shape == want.shape == (1000, 4) and np.array_equal(got, want)
    assert len(np.unique(got)) > 3990                # words, not constants
