"""ktf.egs without a GPU: the generator (the restatement of tests/_egs_ref.py and the library's host entry point) on the published
known answers, the C-ABI of include/ktf_egs.h (symbols, every refusal before any launch), the index, filter and holdout on a bank
written out by hand, the length table, the draw rules and their statistics on the oracle, sharding over ranks, state_dict and the
argument checks of FeatureBank / ChunkSampler."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, egs as E, ops  # noqa: E402
import _egs_ref as R  # noqa: E402

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# 4 speakers, 9 utterances, ties in both orderings: a and c tie on their longest utterance (80), utterances 2 / 6 and 1 / 4 tie in length
HAND_LENS = [50, 80, 70, 80, 80, 30, 70, 60, 20]
HAND_SPK = ["a", "b", "a", "c", "b", "d", "a", "c", "b"]
HAND_LABELS = [0, 1, 0, 2, 1, 3, 0, 2, 1]


def hand_view():
    row0 = np.concatenate([[0], np.cumsum(HAND_LENS)[:-1]])
    return E.BankView(row0, HAND_LENS, HAND_LABELS, ["a", "b", "c", "d"])


# ----------------------------------------------------------------------------- the generator
def test_philox_known_answers_in_the_restatement_and_the_library():
    for ctr, key, want in KNOWN:
        assert R.philox(ctr, key) == want
        assert ops.egs_philox(ctr, key) == want


def test_philox_restatement_equals_the_library_on_random_counters():
    rng = np.random.default_rng(7)
    words = rng.integers(0, 1 << 32, size=(1000, 6), dtype=np.uint64)
    for w in words:
        ctr, key = tuple(int(v) for v in w[:4]), tuple(int(v) for v in w[4:])
        assert R.philox(ctr, key) == ops.egs_philox(ctr, key), (ctr, key)


def test_idx_is_the_bounded_draw():
    assert R.idx(0, 7) == E.idx(0, 7) == 0 and R.idx(0xffffffff, 7) == E.idx(0xffffffff, 7) == 6
    assert R.idx(0x80000000, 5) == 2 and R.idx(0xffffffff, 1) == 0 and R.idx(0xffffffff, (1 << 31) - 1) == (1 << 31) - 2


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_egs_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_egs.h")).read()
    code = hdr[hdr.index("#ifndef KTF_EGS_H_"):]
    protos = re.findall(r"^(?:int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.EGS_PROTOTYPES) == set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", code))
    u32p = C.POINTER(C.c_uint32)
    ctype = {"const KtfEgsIndex*": C.POINTER(L.EgsIndex), "const uint32_t*": u32p, "uint32_t*": u32p, "const void*": L._P, "void*": L._P,
             "const int64_t*": L._P, "const int32_t*": L._P, "int32_t*": L._P, "float*": L._P, "int64_t": L._i64, "int32_t": L._i32,
             "uint64_t": L._u64}
    for name, args in protos:
        args = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert L.EGS_PROTOTYPES[name][1] == [ctype[a.rsplit(" ", 1)[0]] for a in args], name
    assert all(n.startswith("ktf_egs_") for n in L.EGS_PROTOTYPES)
    lib = L.load()
    for name, (res, args) in L.EGS_PROTOTYPES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args, name
    others = (set(L.PROTOTYPES) | set(L.AUGMENT_PROTOTYPES) | set(L.RESAMPLE_PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.NORM_PROTOTYPES)
              | set(L.LOSS_PROTOTYPES))
    assert not set(L.EGS_PROTOTYPES) & others
    for other in ("ktf_hip.h", "ktf_augment.h", "ktf_resample.h", "ktf_grad.h", "ktf_norm.h", "ktf_loss.h"):
        assert "ktf_egs_" not in open(os.path.join(ROOT, "include", other)).read()
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117
    assert int(re.search(r"#define KTF_F16 (\d+)", hdr).group(1)) == L.KTF_F16 == ops.EGS_DTYPES[torch.float16]
    assert ops.EGS_DTYPES[torch.float32] == L.KTF_F32 == 0
    assert int(re.search(r"#define KTF_EGS_THREADS (\d+)", hdr).group(1)) == L.EGS_THREADS
    assert int(re.search(r"#define KTF_EGS_MAX_SLICES (\d+)", hdr).group(1)) == L.EGS_MAX_SLICES
    fields = re.search(r"typedef struct \{(.*?)\} KtfEgsIndex;", hdr, flags=re.S).group(1)
    assert re.findall(r"const int32_t\* (\w+);", fields) == [f for f, _ in L.EgsIndex._fields_]
    assert ktf.egs is E


def _refused(rc, text):
    assert rc == -1, rc
    assert text in L.last_error(), L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")


def test_argument_checks_without_gpu():
    lib = L.load()
    raw = (C.c_float * 65536)()
    buf = C.c_void_p(C.addressof(raw))                 # stands for any non-null device pointer: every refusal comes before a launch
    far = C.c_void_p(buf.value + 131072)               # the bank: 4 rows x 8 floats here, not overlapping B * T * ldo floats at buf
    big = 1 << 31
    index = L.EgsIndex(buf.value, buf.value, buf.value, buf.value)

    def draw(index=index, S=3, U=5, n_spk=2, seed=1, step=2, T=4, b0=0, b_stride=1, B=6, utt=buf, offset=buf, label=buf):
        return lib.ktf_egs_draw(None if index is None else C.byref(index), S, U, n_spk, seed, step, T, b0, b_stride, B, utt, offset, label, None)

    def gather(bank=far, dtype=0, rows=4, ldb=8, D=8, row0=buf, len=buf, U=5, utt=buf, offset=buf, T=4, B=6, out=buf, ldo=8):
        return lib.ktf_egs_gather(bank, dtype, rows, ldb, D, row0, len, U, utt, offset, T, B, out, ldo, None)

    def sample(index=index, S=3, U=5, n_spk=2, seed=1, step=2, T=4, b0=0, b_stride=1, B=6, bank=far, dtype=0, rows=4, ldb=8, D=8, row0=buf,
               len=buf, out=buf, ldo=8, utt=buf, offset=buf, label=buf):
        return lib.ktf_egs_sample(None if index is None else C.byref(index), S, U, n_spk, seed, step, T, b0, b_stride, B, bank, dtype, rows,
                                  ldb, D, row0, len, out, ldo, utt, offset, label, None)

    for fn in (draw, sample):
        for name in ("index", "utt", "offset", "label"):
            _refused(fn(**{name: None}), "null")
        for f, _ in L.EgsIndex._fields_:
            part = L.EgsIndex(buf.value, buf.value, buf.value, buf.value)
            setattr(part, f, None)
            _refused(fn(index=part), "null")
        _refused(fn(T=0), "T 0 below 1")
        _refused(fn(B=-1), "negative")
        _refused(fn(S=0, n_spk=0), "below 1")
        _refused(fn(U=0), "below 1")
        _refused(fn(n_spk=0), "n_spk")
        _refused(fn(n_spk=4), "n_spk")
        _refused(fn(b_stride=0), "b_stride")
        _refused(fn(b0=-1), "b0")
        _refused(fn(b0=big), "last global row")
        _refused(fn(b0=big - 5), "last global row")              # the last of 6 rows is 2^31
        _refused(fn(b0=0, b_stride=big // 5 + 1), "last global row")
        for name in ("B", "T", "S", "U"):
            _refused(fn(**{name: big}), "2^31")
    for fn in (gather, sample):
        for name in ("bank", "row0", "len", "out") + (("utt", "offset") if fn is gather else ()):
            _refused(fn(**{name: None}), "null")
        _refused(fn(D=0, ldb=8), "D 0 below 1")
        _refused(fn(T=0), "T 0 below 1")
        _refused(fn(B=-1), "negative")
        _refused(fn(rows=-1), "negative")
        _refused(fn(U=0), "below 1")
        _refused(fn(ldb=7), "leading dimension")
        _refused(fn(ldo=7), "leading dimension")
        for dtype in (1, 3, -1, 4):
            _refused(fn(dtype=dtype), "dtype")
        for name in ("B", "T", "D", "ldb", "ldo", "U"):
            _refused(fn(**{name: big}), "2^31")
        _refused(fn(B=1 << 16, T=1 << 15), "B * T")
        # out overlapping the bank: the same pointer, the bank's last element, and out's last element at the bank's first
        _refused(fn(bank=buf), "overlaps")
        _refused(fn(out=C.c_void_p(far.value + 4 * (4 * 8 - 1))), "overlaps")
        _refused(fn(out=C.c_void_p(far.value - 4 * (6 * 4 * 8 - 1))), "overlaps")
        _refused(fn(bank=C.c_void_p(buf.value + 2 * 2), dtype=2), "overlaps")
    _refused(lib.ktf_egs_philox(None, None, None), "null")

    # B = 0 is not refused and launches nothing; an empty out or an empty bank overlaps nothing
    assert draw(B=0) == 0 and sample(B=0) == 0 and gather(B=0) == 0
    assert gather(B=0, bank=buf) == 0 and sample(B=0, rows=0, bank=buf) == 0


# ----------------------------------------------------------------------------- the index, filter, holdout
def test_index_of_the_hand_written_bank():
    v = hand_view()
    ix = v.index()
    want = {"spk_order": [1, 2, 0, 3], "spk_off": [0, 3, 6, 8, 9], "spk_utts": [2, 6, 0, 1, 4, 8, 3, 7, 5],
            "spk_utt_len": [70, 70, 50, 80, 80, 20, 80, 60, 30], "spk_max_len": [70, 80, 80, 30]}
    ref = R.build_index(HAND_LENS, HAND_LABELS, 4)
    for k, w in want.items():
        assert ix[k].dtype == np.int32 and list(ix[k]) == w == list(ref[k]), k
    assert (v.num_speakers, v.num_utts, v.num_frames, v.max_len) == (4, 9, sum(HAND_LENS), 80)
    assert [v.eligible_speakers(T) for T in (1, 30, 31, 70, 71, 80, 81)] == [4, 4, 3, 3, 2, 2, 0]
    assert [R.eligible_speakers(ref, T) for T in (1, 30, 31, 70, 71, 80, 81)] == [4, 4, 3, 3, 2, 2, 0]


def test_index_with_a_speaker_without_utterances():
    v = E.BankView([0, 5], [5, 7], [2, 0], ["x", "y", "z"])
    ix, ref = v.index(), R.build_index([5, 7], [2, 0], 3)
    for k in ref:
        assert list(ix[k]) == list(ref[k]), k
    assert list(ix["spk_order"]) == [0, 2, 1] and list(ix["spk_off"]) == [0, 1, 1, 2] and v.eligible_speakers(1) == 2


def test_filter_drops_short_utterances_then_small_speakers():
    v = hand_view()
    f = v.filter(min_frames=50, min_utts_per_speaker=2)              # 5 and 8 are short; d has none left
    assert f.utt_ids == [0, 1, 2, 3, 4, 6, 7] and list(f.labels) == [0, 1, 0, 2, 1, 0, 2] and f.speaker_ids == ["a", "b", "c"]
    assert list(f.row0) == [int(v.row0[u]) for u in f.utt_ids] and list(f.lens) == [HAND_LENS[u] for u in f.utt_ids]
    f = v.filter(min_frames=70, min_utts_per_speaker=2)              # c has two utterances, but only one of 70: the order of the steps
    assert f.utt_ids == [1, 2, 4, 6] and list(f.labels) == [1, 0, 1, 0] and f.speaker_ids == ["a", "b"]
    f = v.filter(min_frames=75, min_utts_per_speaker=2)              # only b survives, renumbered to 0
    assert f.utt_ids == [1, 4] and list(f.labels) == [0, 0] and f.speaker_ids == ["b"] and f.num_speakers == 1
    f = v.filter(min_frames=1, min_utts_per_speaker=1)
    assert f.utt_ids == list(range(9)) and f.speaker_ids == ["a", "b", "c", "d"]
    f = v.filter()                                                   # the recipe's defaults: nothing here is 400 frames long
    assert f.num_utts == 0 and f.num_speakers == 0 and f.max_len == 0 and f.num_frames == 0
    assert v.num_utts == 9                                           # a view is new arrays: the bank's own are as they were


def test_holdout_never_takes_a_speakers_last_utterance():
    v = hand_view()
    for seed in (0, 1, 2 ** 63 + 5):
        train, held = v.holdout(5, seed)
        assert sorted(train.utt_ids + held.utt_ids) == list(range(9)) and held.num_utts == 5
        assert train.speaker_ids == held.speaker_ids == v.speaker_ids
        assert set(train.labels) == {0, 1, 2, 3}                     # 9 utterances of 4 speakers: 5 held out leaves one each
        assert [HAND_LABELS[u] for u in held.utt_ids] == list(held.labels) and 5 not in held.utt_ids
        # the rule, restated
        left, want = list(range(9)), []
        for j in range(5):
            cand = [u for u in left if sum(1 for w in left if HAND_LABELS[w] == HAND_LABELS[u]) >= 2]
            want.append(cand[R.idx(R.philox((j, 0, 0, 2), R.words(seed))[0], len(cand))])
            left.remove(want[-1])
        assert held.utt_ids == sorted(want)
        again = v.holdout(5, seed)[1]
        assert again.utt_ids == held.utt_ids
    assert v.holdout(3, 0)[1].utt_ids != v.holdout(3, 1)[1].utt_ids or v.holdout(3, 0)[1].utt_ids != v.holdout(3, 2)[1].utt_ids
    with pytest.raises(ValueError, match="last one"):
        v.holdout(6, 0)
    train, held = v.holdout(0, 0)
    assert train.utt_ids == list(range(9)) and held.num_utts == 0 and held.num_speakers == 4


# ----------------------------------------------------------------------------- lengths
def test_length_table():
    assert E.length_table(200, 400, 5) == R.length_table(200, 400, 5) == [200, 238, 283, 336, 400]
    assert E.length_table(200, 400, 1) == R.length_table(200, 400, 1) == [400]
    assert E.length_table(300, 300, 4) == [300] and E.length_table(1, 2, 2) == [1, 2]
    s = E.ChunkSampler(hand_view(), 4, min_frames=20, max_frames=80, num_lengths=4, seed=9)
    assert s.lengths == R.length_table(20, 80, 4)
    seen = set()
    for step in (0, 1, 2, 3, 4, 5, 6, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 63):
        assert s.chunk_length(step) == R.chunk_length(s.lengths, 9, step)
        seen.add(s.chunk_length(step))
    assert len(seen) > 1


# ----------------------------------------------------------------------------- the draw rules on the oracle
def test_a_draw_never_selects_an_utterance_shorter_than_T():
    # speakers 0 and 3 have nothing of T = 64 rows; 1 has exactly one, of exactly 64 (its offset must be 0); 2 has two longer ones
    lens = [10, 63, 64, 5, 130, 65, 20, 63, 63]
    labels = [0, 0, 1, 1, 2, 2, 2, 3, 3]
    ix, T = R.build_index(lens, labels, 4), 64
    n_spk = R.eligible_speakers(ix, T)
    assert n_spk == 2
    utt, off, lab = R.draw(ix, 4, 9, n_spk, 3, 11, T, 0, 1, 2000)
    assert set(utt) == {2, 4, 5} and (lab == np.array(labels)[utt]).all()
    assert (off[utt == 2] == 0).all() and set(off[utt == 5]) == {0, 1} and off[utt == 4].max() == 66 and off.min() == 0
    assert (off + T <= np.array(lens)[utt]).all()
    # n_spk too large reaches the speakers without an eligible utterance: those rows are (-1, 0, -1), the others are valid draws
    utt, off, lab = R.draw(ix, 4, 9, 4, 3, 11, T, 0, 1, 2000)
    bad = utt == -1
    assert 0 < bad.sum() < 2000 and (off[bad] == 0).all() and (lab[bad] == -1).all()
    assert set(utt[~bad]) == {2, 4, 5} and (off[~bad] + T <= np.array(lens)[utt[~bad]]).all()


def test_draw_statistics_of_the_oracle():
    """200 000 oracle draws on 5 eligible speakers with 1 - 4 eligible utterances each (and shorter ones, and a sixth speaker with
    none): every (speaker, utterance) cell count and every offset decile within 5 sigma of its binomial expectation."""
    T, N = 100, 200000
    per = [[400], [300, 250], [100, 199, 99], [150, 120, 101, 100], [500, 100, 50, 20], [99, 10]]
    lens = [n for ls in per for n in ls]
    labels = [s for s, ls in enumerate(per) for _ in ls]
    ix = R.build_index(lens, labels, 6)
    n_spk = R.eligible_speakers(ix, T)
    assert n_spk == 5
    utt, off, lab = R.draw(ix, 6, len(lens), n_spk, 20261020, 0, T, 0, 1, N)
    cells = {}
    for s in range(5):
        ok = [u for u in range(len(lens)) if labels[u] == s and lens[u] >= T]
        assert 1 <= len(ok) <= 4
        for u in ok:
            cells[u] = 1.0 / (5 * len(ok))
    assert set(utt) == set(cells) and sorted(len([u for u in cells if labels[u] == s]) for s in range(5)) == [1, 2, 2, 2, 4]
    for u, p in cells.items():
        n = int((utt == u).sum())
        assert abs(n - N * p) <= 5 * np.sqrt(N * p * (1 - p)), (u, n, N * p)
    # the offset within its utterance's range, as a fraction: deciles (the utterances of exactly T rows have the single offset 0)
    room = np.array(lens)[utt] - T + 1
    free = room > 1
    dec = np.minimum((off[free] * 10) // room[free], 9)
    exact = np.zeros(10)
    for u in cells:
        r = lens[u] - T + 1
        if r > 1:
            exact += cells[u] * np.bincount(np.minimum((np.arange(r) * 10) // r, 9), minlength=10) / r
    n_free = int(free.sum())
    p = exact / exact.sum()
    for d in range(10):
        n = int((dec == d).sum())
        assert abs(n - n_free * p[d]) <= 5 * np.sqrt(n_free * p[d] * (1 - p[d])), (d, n, n_free * p[d])


@pytest.mark.parametrize("W", [2, 4])
def test_the_ranks_together_are_the_world_of_one(W):
    v = hand_view()
    ix, B, T, seed, step = R.build_index(HAND_LENS, HAND_LABELS, 4), 16, 50, 5, 3
    whole = E.ChunkSampler(v, B, 50, 50, seed=seed)
    assert whole.global_rows() == (0, 1, B) and whole.chunk_length(step) == T
    want = R.draw(ix, 4, 9, v.eligible_speakers(T), seed, step, T, *whole.global_rows())
    assert len(set(zip(*[list(a) for a in want]))) > 4
    got = [np.zeros(B, np.int32) for _ in range(3)]
    for r in range(W):
        s = E.ChunkSampler(v, B, 50, 50, seed=seed, rank=r, world=W)
        b0, stride, n = s.global_rows()
        assert (b0, stride, n) == (r, W, B // W)
        part = R.draw(ix, 4, 9, v.eligible_speakers(T), seed, step, T, b0, stride, n)
        for g, p in zip(got, part):
            g[b0::stride] = p
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ----------------------------------------------------------------------------- the Python layer's own checks
def test_state_dict_round_trip():
    v = hand_view()
    a = E.ChunkSampler(v, 4, 20, 80, seed=2 ** 40 + 3)
    a.step = 2 ** 33 + 1
    state = a.state_dict()
    assert state == {"seed": 2 ** 40 + 3, "step": 2 ** 33 + 1}
    b = E.ChunkSampler(v, 4, 20, 80, seed=0)
    b.load_state_dict(state)
    assert b.state_dict() == state and b.chunk_length(b.step) == a.chunk_length(a.step)
    with pytest.raises(ValueError):
        b.load_state_dict({"seed": -1, "step": 0})
    with pytest.raises(ValueError):
        b.load_state_dict({"seed": 0, "step": 2 ** 64})


def test_sampler_value_errors():
    v = hand_view()
    with pytest.raises(ValueError, match="no speaker is eligible"):
        E.ChunkSampler(v, 4, 20, 81)
    with pytest.raises(ValueError, match="min_frames"):
        E.ChunkSampler(v, 4, 60, 50)
    with pytest.raises(ValueError, match="min_frames"):
        E.ChunkSampler(v, 4, 0, 50)
    with pytest.raises(ValueError, match="num_lengths"):
        E.ChunkSampler(v, 4, 20, 50, num_lengths=0)
    with pytest.raises(ValueError, match="does not divide"):
        E.ChunkSampler(v, 6, 20, 50, world=4)
    with pytest.raises(ValueError, match="rank"):
        E.ChunkSampler(v, 4, 20, 50, rank=2, world=2)
    with pytest.raises(ValueError, match="64-bit"):
        E.ChunkSampler(v, 4, 20, 50, seed=-1)
    with pytest.raises(ValueError):
        E.ChunkSampler(v.filter(), 4)                                # an empty view: its longest utterance is 0 rows
    with pytest.raises(ValueError):
        E.BankView([0, 1], [1], [0], ["a"])
    with pytest.raises(ValueError):
        E.BankView([0], [1], [1], ["a"])
    with pytest.raises(ValueError):
        ops.egs_index(*[torch.zeros(2, dtype=torch.int64)] * 4)


def test_the_gpu_is_required_where_the_kernels_run():
    s = E.ChunkSampler(hand_view(), 4, 20, 50)
    for call in (lambda: s.batch(0), lambda: s.plan(0), lambda: next(s), lambda: s.gather([0], [0], 5)):
        with pytest.raises(ktf.KtfBackendError):                     # a view without a bank on the GPU
            call()
    with pytest.raises(ValueError):
        E.FeatureBank(4, 10, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        E.FeatureBank(0, 10)
    with pytest.raises(ktf.KtfBackendError):                         # without a GPU the bank itself; with one, the tensors on the CPU
        E.FeatureBank(4, 10, device="cpu")
    with pytest.raises(ktf.KtfBackendError):
        E.FeatureBank(4, 10).add(torch.zeros(1, 3, 4), torch.tensor([3], dtype=torch.int32), ["a"])
