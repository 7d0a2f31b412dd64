"""The index arithmetic of the chunked row walk (egc_amd/csrc/egc_row_chunks.h: slot count, slot -> chunk lookup, a row's
clamped range and partial range) run on the host by tests/row_chunks/row_chunks_check.cpp and checked here against the CSR.
A chunk kernel stores to workspace slot g with nothing but g < slots in front of it, and a row kernel reads slots
first .. first + n_part - 1: every chunk k >= 1 of a row must be one slot's, that slot the one the row reads, and below
the slot count."""
import os
import subprocess

import numpy as np
import pytest

import mpnn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "row_chunks", "_build", "row_chunks_check")
CHUNK = mpnn_ref.CHUNK


def _rowptr(lengths):
    return [0] + [int(v) for v in np.cumsum(np.asarray(lengths, dtype=np.int64))]


WELL_FORMED = {
    "ladder": _rowptr(mpnn_ref.ladder_lengths()),
    "ladder_pad_to_chunk": _rowptr(mpnn_ref.ladder_lengths(pad_to_chunk=True)),
    "ladder_tail_empty": _rowptr(mpnn_ref.ladder_lengths(tail_empty=True)),
    "ladder_prepend_3": _rowptr(mpnn_ref.ladder_lengths(prepend=3)),
    "one_row_of_chunk": _rowptr([CHUNK]),
    "one_row_of_chunk_plus_1": _rowptr([CHUNK + 1]),
    "one_row_of_100000": _rowptr([100000]),
}
# (rowptr, n_edges): offsets that decrease, that are negative, that pass the entry count
MALFORMED = {
    "decreasing": ([0, 3 * CHUNK, CHUNK, 2 * CHUNK + 7, 5 * CHUNK], 5 * CHUNK),
    "negative": ([0, -5, 2 * CHUNK + 3, -CHUNK, 4 * CHUNK + 1], 4 * CHUNK + 1),
    "past_n_edges": ([0, CHUNK + 9, 7 * CHUNK, 9 * CHUNK + 5, 3 * CHUNK], 3 * CHUNK),
}


@pytest.fixture(scope="module")
def reports():
    """name -> rowptr, n_edges, slots (the count), found {slot: (row, s0, s1)}, rows [(p0, p1, first, n_part)]: ONE run of the
    program over every CSR of this file."""
    subprocess.run(["bash", os.path.join(ROOT, "tests", "row_chunks", "build.sh")], check=True, capture_output=True)
    cases = [(k, v, v[-1]) for k, v in WELL_FORMED.items()] + [(k, v[0], v[1]) for k, v in MALFORMED.items()]
    text = "".join(f"{len(rp) - 1} {e}\n{' '.join(map(str, rp))}\n" for _, rp, e in cases)
    r = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == f"chunk {CHUNK}"
    out, cur = {}, None
    for w in (line.split() for line in lines[1:] if line):
        if w[0] == "csr":
            name, rp, e = cases[int(w[1])]
            cur = out[name] = {"rowptr": rp, "n_edges": e, "slots": None, "listed": [], "found": {}, "rows": []}
        elif w[0] == "slots":
            cur["slots"] = int(w[1])
        elif w[0] == "slot":
            cur["listed"].append(int(w[1]))
            if w[2] != "none":
                cur["found"][int(w[1])] = tuple(int(x) for x in w[2:5])
        else:
            assert w[0] == "row" and int(w[1]) == len(cur["rows"])
            cur["rows"].append(tuple(int(x) for x in w[2:6]))
    assert list(out) == [c[0] for c in cases]
    for name, c in out.items():                                                      # one line per slot, one per row
        assert c["listed"] == list(range(c["slots"])) and len(c["rows"]) == len(c["rowptr"]) - 1, name
    return out


@pytest.mark.parametrize("name", list(WELL_FORMED))
def test_every_later_chunk_is_one_slot_and_the_slot_the_row_reads(reports, name):
    c = reports[name]
    rp, e, slots, found, rows = c["rowptr"], c["n_edges"], c["slots"], c["found"], c["rows"]
    assert slots == (-(-e // CHUNK) if e > CHUNK else 0)
    expected = {}
    for r in range(len(rp) - 1):
        p0, p1 = rp[r], rp[r + 1]
        n_later = (p1 - p0 - 1) // CHUNK if p1 - p0 > CHUNK else 0
        assert rows[r] == (p0, p1, (p0 + CHUNK) // CHUNK, n_later), (name, r)
        first = rows[r][2]
        for k in range(1, n_later + 1):
            start = p0 + k * CHUNK
            slot = start // CHUNK
            assert slot == first + k - 1 and slot < slots and slot not in expected, (name, r, k)
            expected[slot] = (r, start, min(start + CHUNK, p1))
    assert found == expected, name                                                   # these slots and no other
    for row, s0, s1 in found.values():
        assert 0 < s1 - s0 <= CHUNK and s1 <= rp[row + 1]
    if name == "one_row_of_100000":
        assert len(found) == 390 and slots == 391
    if name == "one_row_of_chunk":
        assert slots == 0 and rows == [(0, CHUNK, 1, 0)]
    if name == "one_row_of_chunk_plus_1":
        assert slots == 2 and found == {1: (0, CHUNK, CHUNK + 1)}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_offsets_give_ranges_inside_the_entries(reports, name):
    c = reports[name]
    rp, e, slots, found, rows = c["rowptr"], c["n_edges"], c["slots"], c["found"], c["rows"]
    assert slots == -(-e // CHUNK)
    for slot, (row, s0, s1) in found.items():
        assert 0 <= slot < slots and 0 <= row < len(rp) - 1 and 0 <= s0 < s1 <= e, (name, slot)
    for p0, p1, first, n_part in rows:
        assert 0 <= p0 <= p1 <= e and n_part >= 0 and (n_part == 0 or first + n_part <= slots), name
