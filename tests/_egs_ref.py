"""The rules of include/ktf_egs.h restated in Python integers and numpy, for the tests: Philox4x32-10, the bounded draw, the index,
rules 1 - 7 (the draw and what a violated precondition gives), the length table and the gather. Nothing here calls the library."""

import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(ctr, key):
    """Philox4x32-10: ctr four, key two 32-bit words -> four 32-bit words."""
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def idx(r, n):
    return (int(r) * int(n)) >> 32


def words(v):
    return int(v) & MASK, int(v) >> 32


def build_index(lens, labels, S):
    """The index of ktf_egs.h from per-utterance lengths and labels, by plain sorting."""
    lens, labels = [int(v) for v in lens], [int(v) for v in labels]
    per = [sorted((u for u in range(len(lens)) if labels[u] == s), key=lambda u: (-lens[u], u)) for s in range(S)]
    longest = [max((lens[u] for u in us), default=0) for us in per]
    off = [0]
    for us in per:
        off.append(off[-1] + len(us))
    utts = [u for us in per for u in us]
    return {"spk_order": sorted(range(S), key=lambda s: (-longest[s], s)), "spk_off": off, "spk_utts": utts,
            "spk_utt_len": [lens[u] for u in utts], "spk_max_len": longest}


def eligible_speakers(index, T):
    return sum(1 for v in index["spk_max_len"] if v >= T)


def draw_row(index, S, U, n_spk, seed, step, T, b):
    """Rules 1 - 7 for global row b: (utt, offset, label)."""
    r0, r1, r2, _ = philox((b,) + words(step) + (0,), words(seed))
    s = index["spk_order"][idx(r0, n_spk)]
    if not 0 <= s < S:
        return -1, 0, -1
    first, last = index["spk_off"][s], index["spk_off"][s + 1]
    if first < 0 or last < first or last > U:
        return -1, 0, -1
    ul = index["spk_utt_len"][first:last]
    m = sum(1 for v in ul if v >= T)
    if m == 0:
        return -1, 0, -1
    k = idx(r1, m)
    u = index["spk_utts"][first + k]
    if not 0 <= u < U or ul[k] < T:
        return -1, 0, -1
    return u, idx(r2, ul[k] - T + 1), s


def draw(index, S, U, n_spk, seed, step, T, b0, b_stride, B):
    """(utt, offset, label) int32 (B,) for the global rows b0 + i * b_stride."""
    rows = [draw_row(index, S, U, n_spk, seed, step, T, b0 + i * b_stride) for i in range(B)]
    return tuple(np.array([r[k] for r in rows], np.int32).reshape(B) for k in range(3))


def plan_ok(row0, lens, rows, u, off, T):
    """Rule 7 for a plan row."""
    if not 0 <= u < len(lens) or off < 0:
        return False
    return off + T <= lens[u] and row0[u] >= 0 and row0[u] + lens[u] <= rows


def gather(bank, D, row0, lens, utt, offset, T, ldo):
    """out (B, T, ldo) fp32 of rule 8 from bank (rows, >= D) fp32 / fp16; rule 7 for the rows the plan gets wrong."""
    out = np.zeros((len(utt), T, ldo), np.float32)
    for i, (u, off) in enumerate(zip(utt, offset)):
        if plan_ok(row0, lens, bank.shape[0], int(u), int(off), T):
            first = int(row0[u]) + int(off)
            out[i, :, :D] = bank[first:first + T, :D].astype(np.float32)
    return out


def length_table(lo, hi, n):
    if n == 1 or lo == hi:
        return [hi]
    return [int(math.floor(lo * (hi / lo) ** (i / (n - 1)) + 0.5)) for i in range(n)]


def chunk_length(table, seed, step):
    return table[idx(philox((0,) + words(step) + (1,), words(seed))[0], len(table))]
