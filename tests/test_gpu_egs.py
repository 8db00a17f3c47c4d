"""ktf.egs on the GPU, bit for bit against the restatement of tests/_egs_ref.py (there is no arithmetic, so no tolerance): the draw
on every T / B / shard / step of the issue, the gather on every D / dtype / leading dimension / element offset with NaN around the
bank and sentinels around the output, the one-launch sample against draw + gather, what a violated precondition gives, the
Python layer (FeatureBank, ChunkSampler) and three training steps from wavs."""

import functools
import itertools
import os
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
from kaldi_tflite_amd import autograd as A, egs as E, ops  # noqa: E402
import _egs_ref as R  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25

# 7 speakers, 23 utterances, lengths in {1, 2, 5, 64, 65, 130}; ties in both orderings of the index
_PER_SPEAKER = [[130, 65, 64, 5, 2, 1], [130, 130, 64], [65, 65, 5], [64, 2, 1, 1], [5, 5, 2], [1], [130, 64, 65]]
_ORDER = np.random.default_rng(23).permutation(23)                # the utterances are not grouped by speaker
LENS = [0] * 23
LABELS = [0] * 23
for _k, (_s, _n) in enumerate((s, n) for s, ls in enumerate(_PER_SPEAKER) for n in ls):
    LENS[_ORDER[_k]], LABELS[_ORDER[_k]] = _n, _s
S, U = 7, 23
LAST = int(np.argmax(np.array(LENS) == 130))                      # this utterance is put last: it ends on the bank's last row
ROW0 = [0] * U
_r = 0
for _u in [u for u in range(U) if u != LAST] + [LAST]:
    _r += _u % 3                                                  # 0 - 2 rows no utterance owns in front of each
    ROW0[_u] = _r
    _r += LENS[_u]
ROWS = _r
INDEX = R.build_index(LENS, LABELS, S)
TS = [1, 2, 5, 64, 65, 130]
BS = [1, 3, 64, 257]
SHARDS = [(0, 1), (1, 2), (3, 4)]
STEPS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63]
SEED = 0x9E3779B97F4A7C15


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _i32(a):
    return torch.as_tensor(np.asarray(a, np.int32), device=DEV)


@functools.lru_cache(maxsize=None)
def dev_index():
    t = {k: _i32(INDEX[k]) for k in ("spk_order", "spk_off", "spk_utts", "spk_utt_len")}
    t["row0"] = torch.as_tensor(np.asarray(ROW0, np.int64), device=DEV)
    t["lens"] = _i32(LENS)
    t["index"] = ops.egs_index(t["spk_order"], t["spk_off"], t["spk_utts"], t["spk_utt_len"])
    return t


@functools.lru_cache(maxsize=None)
def bank_values(D, dtype):
    """(ROWS, D) values of the owned rows (elsewhere NaN), with the corner values of the element type in the first of them."""
    rng = np.random.default_rng(1000 + D)
    v = np.full((ROWS, D), np.nan, np.float32)
    for u in range(U):
        v[ROW0[u]:ROW0[u] + LENS[u]] = rng.standard_normal((LENS[u], D)) * 3.0
    special = [-0.0, 65504.0, -65504.0, 6e-8, 6.1e-5, np.inf] if dtype == np.float16 else [-0.0, 3.4e38, 1e-45, 1.17e-38, -np.inf, 1 / 3]
    first = ROW0[int(np.argmax(np.array(LENS) == 64))]
    v[first:first + len(special), 0] = special
    return v.astype(dtype)


def make_bank(D, dtype, ldb, off):
    """The bank as a (ROWS, D) view with row stride ldb at element offset `off` of a NaN-filled tensor, and the same on the host."""
    vals = bank_values(D, dtype)
    flat = np.full(off + ROWS * ldb + 8, np.nan, dtype)
    flat[off:off + ROWS * ldb].reshape(ROWS, ldb)[:, :D] = vals
    t = torch.as_tensor(flat, device=DEV)
    return t[off:off + ROWS * ldb].view(ROWS, ldb)[:, :D], vals


def make_out(B, T, D, ldo, off):
    """out (B, T, D) as a view with row stride ldo at element offset `off` of a sentinel-filled tensor, and that tensor."""
    if B == 1 and T == 1:
        ldo = D                                                   # a single row has no stride to show
    flat = torch.full((off + B * T * ldo + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    return flat[off:off + B * T * ldo].view(B, T, ldo)[:, :, :D], flat, ldo


def check_out(flat, off, B, T, ldo, want, tag):
    """The (B, T, ldo) block of `flat` equals `want` bit for bit (its pad columns are zeros) and the sentinels around it stand."""
    got = flat.cpu().numpy()
    n = B * T * ldo
    assert np.array_equal(_bits(got[off:off + n]).reshape(B, T, ldo), _bits(want)), tag
    assert (got[:off] == SENTINEL).all() and (got[off + n:] == SENTINEL).all(), tag


def full_plan(T):
    """Every utterance of at least T rows at its first, its last and a middle offset; the last row is the bank's last owned one."""
    utt, off = [], []
    for u in range(U):
        if LENS[u] >= T:
            for o in sorted({0, (LENS[u] - T) // 2, LENS[u] - T}):
                utt.append(u)
                off.append(o)
    assert any(ROW0[u] + o + T == ROWS for u, o in zip(utt, off))
    return utt, off


def lds(D):
    return sorted({D, D + 1, ops.round_up(D, 32)})


# ----------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("shard", SHARDS)
@pytest.mark.parametrize("T", TS)
def test_draw_equals_the_oracle(T, shard):
    d = dev_index()
    n_spk = R.eligible_speakers(INDEX, T)
    assert n_spk >= 1
    b0, stride = shard
    seen = set()
    for B, step in itertools.product(BS, STEPS):
        utt, off, lab = (torch.full((B,), -5, dtype=torch.int32, device=DEV) for _ in range(3))
        ops.egs_draw(d["index"], S, U, n_spk, SEED, step, T, b0, stride, utt, off, lab)
        want = R.draw(INDEX, S, U, n_spk, SEED, step, T, b0, stride, B)
        for g, w, name in zip((utt, off, lab), want, ("utt", "offset", "label")):
            assert np.array_equal(g.cpu().numpy(), w), (name, T, B, shard, step)
        assert (want[0] >= 0).all() and (np.array(LENS)[want[0]] >= T).all()
        seen.add(tuple(want[0][:3]))
    assert len(seen) > 1 or n_spk == 1                                # the step reaches the draw, in its low and its high word


def test_draw_does_not_depend_on_the_batch_shape():
    d = dev_index()
    T, n_spk = 5, R.eligible_speakers(INDEX, 5)
    whole = [torch.empty(257, dtype=torch.int32, device=DEV) for _ in range(3)]
    ops.egs_draw(d["index"], S, U, n_spk, SEED, 7, T, 0, 1, *whole)
    for b0, stride in SHARDS:
        n = len(range(b0, 257, stride))
        part = [torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3)]
        ops.egs_draw(d["index"], S, U, n_spk, SEED, 7, T, b0, stride, *part)
        for w, p in zip(whole, part):
            assert torch.equal(w[b0::stride], p)


# ----------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("D", [1, 23, 30, 32, 33])
def test_gather_equals_the_oracle_on_every_stride_and_offset(D, dtype):
    d = dev_index()
    calls = 0
    for ldb, ldo in itertools.product(lds(D), (D, D + 3)):
        for bank_off, out_off, T in itertools.product(range(4), range(4), TS):
            if T != 5 and out_off != (bank_off + 1) % 4:             # the full cross of offsets at T = 5, a pairing at the others
                continue
            bank, vals = make_bank(D, dtype, ldb, bank_off)
            utt, off = full_plan(T)
            B = len(utt)
            out, flat, eff = make_out(B, T, D, ldo, out_off)
            ops.egs_gather(bank, d["row0"], d["lens"], _i32(utt), _i32(off), T, out)
            want = R.gather(vals, D, ROW0, LENS, utt, off, T, eff)
            assert not np.isnan(want).any() and not (want[:, :, D:] != 0).any()
            check_out(flat, out_off, B, T, eff, want, (D, dtype, ldb, ldo, bank_off, out_off, T))
            calls += 1
    assert calls == len(lds(D)) * 2 * (16 + 4 * 5)


def test_gather_more_elements_than_the_slices_take_at_once():
    """T * ldo = 130 * 512 elements is more than KTF_EGS_MAX_SLICES workgroups of 8 * 256 take in one go: their loop comes round."""
    from kaldi_tflite_amd import _lib as L
    D, T, ldo = 509, 130, 512
    assert T * ldo > L.EGS_MAX_SLICES * L.EGS_THREADS * 8
    d = dev_index()
    for dtype in (np.float32, np.float16):
        bank, vals = make_bank(D, dtype, D, 1)
        utt, off = full_plan(T)
        out, flat, eff = make_out(len(utt), T, D, ldo, 3)
        ops.egs_gather(bank, d["row0"], d["lens"], _i32(utt), _i32(off), T, out)
        check_out(flat, 3, len(utt), T, eff, R.gather(vals, D, ROW0, LENS, utt, off, T, eff), dtype)


# ----------------------------------------------------------------------------- the sample
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("D", [1, 23, 30, 32, 33])
def test_sample_equals_draw_then_gather(D, dtype):
    """Every T x B; the shards, steps, leading dimensions and element offsets cycle through their values along the way (each value
    of each is reached several times, not their whole cross)."""
    d = dev_index()
    for k, (T, B) in enumerate(itertools.product(TS, BS)):
        (b0, stride), step = SHARDS[k % 3], STEPS[k % 5]
        ldb, ldo, bank_off, out_off = lds(D)[k % len(lds(D))], (D, D + 3)[(k // 3) % 2], (k + k // 4) % 4, (k // 2) % 4
        tag = (D, dtype, T, B, b0, stride, step, ldb, ldo, bank_off, out_off)
        n_spk = R.eligible_speakers(INDEX, T)
        bank, vals = make_bank(D, dtype, ldb, bank_off)
        plans, flats = [], []
        for _ in range(2):                                           # two calls: the same bits
            out, flat, eff = make_out(B, T, D, ldo, out_off)
            plan = [torch.full((B,), -5, dtype=torch.int32, device=DEV) for _ in range(3)]
            ops.egs_sample(d["index"], S, n_spk, SEED, step, T, b0, stride, bank, d["row0"], d["lens"], out, *plan)
            plans.append(plan)
            flats.append(flat)
        drawn = [torch.full((B,), -6, dtype=torch.int32, device=DEV) for _ in range(3)]
        ops.egs_draw(d["index"], S, U, n_spk, SEED, step, T, b0, stride, *drawn)
        out2, flat2, _ = make_out(B, T, D, ldo, out_off)
        ops.egs_gather(bank, d["row0"], d["lens"], drawn[0], drawn[1], T, out2)
        want = R.draw(INDEX, S, U, n_spk, SEED, step, T, b0, stride, B)
        for a, b, c, w in zip(plans[0], plans[1], drawn, want):
            assert torch.equal(a, b) and torch.equal(a, c) and np.array_equal(a.cpu().numpy(), w), tag
        assert torch.equal(flats[0].view(torch.int32), flats[1].view(torch.int32)), tag
        assert torch.equal(flats[0].view(torch.int32), flat2.view(torch.int32)), tag
        check_out(flats[0], out_off, B, T, eff, R.gather(vals, D, ROW0, LENS, want[0], want[1], T, eff), tag)


# ----------------------------------------------------------------------------- violated preconditions: values, never a fault
def test_a_wrong_plan_row_is_zeros_with_label_minus_one():
    D, T = 30, 5
    bank, vals = make_bank(D, np.float32, D, 0)
    view = E.BankView(ROW0, LENS, LABELS, list(range(S)), storage=bank)
    sampler = E.ChunkSampler(view, 4, 5, 5)
    long_ = [u for u in range(U) if LENS[u] >= 64][:3]
    short = int(np.argmax(np.array(LENS) == 2))
    #       good            utt = -1  utt = U   offset = -1   offset + T = len + 1     good at the end   too short for T
    utt = [long_[0],        -1,       U,        long_[1],     long_[2],                long_[2],         short]
    off = [3,               0,        0,        -1,           LENS[long_[2]] - T + 1,  LENS[long_[2]] - T, 0]
    bad = np.array([False, True, True, True, True, False, True])
    feats, lens, labels = sampler.gather(utt, off, T)
    want = R.gather(vals, D, ROW0, LENS, utt, off, T, D)
    assert np.array_equal(_bits(feats.cpu().numpy()), _bits(want))
    assert not want[bad].any() and all(want[i].any() for i in np.flatnonzero(~bad))
    assert lens.dtype == torch.int32 and lens.tolist() == [T] * 7
    assert labels.dtype == torch.int32 and labels.tolist() == [-1 if b else LABELS[u] for u, b in zip(utt, bad)]

    # an utterance the bank cannot hold (row0 + len beyond its rows, or a negative row0) is not read either
    d = dev_index()
    row0 = np.array(ROW0, np.int64)
    row0[long_[0]], row0[long_[1]] = ROWS - LENS[long_[0]] + 1, -1
    out, flat, _ = make_out(3, T, D, D + 3, 1)
    plan_u, plan_o = [long_[0], long_[1], long_[2]], [0, 0, 1]
    ops.egs_gather(bank, torch.as_tensor(row0, device=DEV), d["lens"], _i32(plan_u), _i32(plan_o), T, out)
    want = R.gather(vals, D, row0, LENS, plan_u, plan_o, T, D + 3)
    assert not want[:2].any() and want[2].any()
    check_out(flat, 1, 3, T, D + 3, want, "row0")


@pytest.mark.parametrize("T", [64, 65, 130])
def test_n_spk_too_large_gives_minus_one_rows_where_the_oracle_says(T):
    d = dev_index()
    D, B = 23, 257
    assert R.eligible_speakers(INDEX, T) < S
    bank, vals = make_bank(D, np.float16, D + 1, 1)
    want = R.draw(INDEX, S, U, S, SEED, 4, T, 0, 1, B)
    bad = want[0] == -1
    assert 0 < bad.sum() < B and (want[1][bad] == 0).all() and (want[2][bad] == -1).all()
    drawn = [torch.full((B,), -5, dtype=torch.int32, device=DEV) for _ in range(3)]
    ops.egs_draw(d["index"], S, U, S, SEED, 4, T, 0, 1, *drawn)
    out, flat, _ = make_out(B, T, D, D, 2)
    plan = [torch.full((B,), -5, dtype=torch.int32, device=DEV) for _ in range(3)]
    ops.egs_sample(d["index"], S, S, SEED, 4, T, 0, 1, bank, d["row0"], d["lens"], out, *plan)
    for a, b, w in zip(drawn, plan, want):
        assert np.array_equal(a.cpu().numpy(), w) and torch.equal(a, b)
    ref = R.gather(vals, D, ROW0, LENS, want[0], want[1], T, D)
    assert not ref[bad].any() and np.abs(ref[~bad]).max() > 0
    check_out(flat, 2, B, T, D, ref, T)


# ----------------------------------------------------------------------------- the Python layer
@pytest.mark.parametrize("store", [torch.float32, torch.float16])
def test_feature_bank_add_and_sampler_against_the_oracle(store):
    D = 30
    rng = np.random.default_rng(5)
    bank = E.FeatureBank(D, 1200, dtype=store, device=DEV)
    spk = ["s%d" % LABELS[u] for u in range(U)]
    kept = []
    for lo, hi, dt in ((0, 8, torch.float32), (8, 16, torch.bfloat16), (16, U, torch.float16)):
        x = torch.as_tensor(rng.standard_normal((hi - lo, 130, D)).astype(np.float32), device=DEV).to(dt)
        bank.add(x, _i32(LENS[lo:hi]), spk[lo:hi])
        kept += [x[b, :LENS[lo + b]].to(store).float().cpu().numpy() for b in range(hi - lo)]
    assert (bank.num_utts, bank.num_frames, bank.max_len) == (U, sum(LENS), 130)
    first_seen = list(dict.fromkeys(spk))
    assert bank.speaker_ids == first_seen and list(bank.labels) == [first_seen.index(s) for s in spk]
    assert list(bank.row0) == list(np.concatenate([[0], np.cumsum(LENS)[:-1]])) and bank.utt_ids == list(range(U))
    host = bank.storage.float().cpu().numpy()
    for u in range(U):
        assert np.array_equal(_bits(host[bank.row0[u]:bank.row0[u] + LENS[u]]), _bits(kept[u]))
    with pytest.raises(ValueError, match="do not fit"):
        bank.add(torch.zeros((1, 1200, D), device=DEV), _i32([1200]), ["x"])
    bank.add(torch.zeros((1, 4, D), device=DEV), _i32([0]), ["never"])                 # an empty utterance adds nothing
    assert bank.num_utts == U and "never" not in bank.speaker_ids

    ix = R.build_index(bank.lens, bank.labels, bank.num_speakers)
    world = E.ChunkSampler(bank, 12, 2, 130, num_lengths=6, seed=3)
    ranks = [E.ChunkSampler(bank, 12, 2, 130, num_lengths=6, seed=3, rank=r, world=3) for r in range(3)]
    lengths = set()
    for step in range(6):
        T = R.chunk_length(R.length_table(2, 130, 6), 3, step)
        lengths.add(T)
        feats, lens, labels = next(world)
        assert world.step == step + 1 and feats.shape == (12, T, D) and feats.dtype == torch.float32 and lens.tolist() == [T] * 12
        want = R.draw(ix, bank.num_speakers, U, R.eligible_speakers(ix, T), 3, step, T, 0, 1, 12)
        plan = world.plan(step)
        for g, w in zip(plan, want):
            assert np.array_equal(g.cpu().numpy(), w)
        assert np.array_equal(labels.cpu().numpy(), want[2]) and labels.dtype == torch.int32
        ref = R.gather(host, D, bank.row0, bank.lens, want[0], want[1], T, D)
        assert np.array_equal(_bits(feats.cpu().numpy()), _bits(ref))
        again = world.gather(plan[0], plan[1], T)
        assert torch.equal(again[0].view(torch.int32), feats.view(torch.int32)) and torch.equal(again[2], labels)
        for r, s in enumerate(ranks):
            f, _, lab = s.batch(step)
            assert torch.equal(f.view(torch.int32), feats[r::3].view(torch.int32)) and torch.equal(lab, labels[r::3])
    assert len(lengths) > 1

    # the ring is two deep: a batch stands through the next call
    a = world.batch(0)
    keep = [t.clone() for t in a]
    world.batch(1)
    assert all(torch.equal(x, y) for x, y in zip(a, keep))


# ----------------------------------------------------------------------------- from wavs to three training steps
def test_wavs_to_three_training_steps_and_a_resumed_sampler():
    cfg = synth.extractor_cfg()
    extractor = synth.build_extractor(ktf, cfg, synth.make_weights(seed=4321, narrow=True), gemm="f32")
    wavs = np.concatenate([synth.speech_wavs(32000)[1], synth.make_wav(6, 32000, seed=77, ragged=True)])
    speakers = ["p", "p", "q", "q", "r", "r", "s", "s"]
    bank = E.FeatureBank(30, 8 * 200, device=DEV).add_wavs(extractor, torch.as_tensor(wavs, device=DEV), speakers)
    assert bank.num_speakers == 4 and bank.num_utts == 8 and bank.max_len >= 80
    view = bank.filter(min_frames=80, min_utts_per_speaker=2)
    assert view.num_speakers >= 2
    Lr, M = ktf.layers, ktf.models
    seq = M.Sequential([M.Input(shape=(None, 30)), Lr.TDNN(32, [-2, -1, 0, 1, 2], name="tdnn1"), Lr.ReLU(name="relu1"),
                        Lr.BatchNorm(name="bn1"), Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"),
                        Lr.TDNN(32, [0], name="affine1")], name="tiny_xvector")
    torch.manual_seed(3)
    net = A.TrainableSequential(seq, fused_norm=True).train()
    head = A.ClassifierHead(32, view.num_speakers, kind="aam", margin=0.2, scale=16.0, device=DEV)
    opt = torch.optim.SGD(list(net.parameters()) + list(head.parameters()), lr=0.05)
    sampler = E.ChunkSampler(view, 8, 40, 80, num_lengths=3, seed=11)
    resumed, batches, losses = None, [], []
    for step, (feats, lens, labels) in zip(range(3), sampler):
        assert int(labels.min()) >= 0 and int(labels.max()) < view.num_speakers and torch.isfinite(feats).all()
        batches.append((feats.clone(), lens.clone(), labels.clone()))
        opt.zero_grad()
        loss, _ = head(net(feats, lens), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if step == 0:
            resumed = E.ChunkSampler(view, 8, 40, 80, num_lengths=3, seed=0)
            resumed.load_state_dict(sampler.state_dict())
    print("losses", losses)
    assert np.isfinite(losses).all()
    for step in (1, 2):
        feats, lens, labels = next(resumed)
        for got, want in zip((feats, lens, labels), batches[step]):
            assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), step
    assert resumed.state_dict() == sampler.state_dict() == {"seed": 11, "step": 3}
