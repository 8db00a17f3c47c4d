"""
Training examples on the GPU (include/ktf_egs.h): a bank of feature rows and random fixed-length chunk
batches drawn from it, the stage of Kaldi's sid/nnet3/xvector recipe (prepare_feats_for_egs.sh, get_egs.sh, allocate_egs.py)
between the front-end and the training step of ktf.autograd.

    bank = ktf.egs.FeatureBank(dim=30, capacity_frames=2_000_000)
    bank.add_wavs(extractor, wavs, speakers)                  # CMVN'd, voiced-only rows straight from the front-end
    train, heldout = bank.filter(400, 8).holdout(1000, seed=1)
    for feats, lens, labels in ktf.egs.ChunkSampler(train, batch_size=64, seed=0):
        loss, _ = head(net(feats, lens), labels)

A batch row is a function of (seed, step, global row) alone (rules 1 - 6 of the header), which is what makes resuming
(`state_dict`) and sharding over ranks (`rank`, `world`) trivial. The host keeps only index arrays; the rows never leave the GPU.
"""

import numpy as np
import torch

from . import _lib as L, ops

HOLDOUT_STREAM, LENGTH_STREAM = 2, 1     # the fourth counter word of the host draws (0: the batch rows of rule 1)
MASK32 = 0xFFFFFFFF


def idx(r, n):
    """The bounded draw of ktf_egs.h from a 32-bit word."""
    return (int(r) * int(n)) >> 32


def _words(v):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f"seed and step are unsigned 64-bit integers, got {v}")
    return v & MASK32, v >> 32


def length_table(min_frames, max_frames, num_lengths):
    """Kaldi's geometric chunk lengths: T_i = floor(min * (max / min)^(i / (L - 1)) + 0.5); `max` alone when L == 1 or min == max."""
    lo, hi, n = int(min_frames), int(max_frames), int(num_lengths)
    if lo < 1 or lo > hi or n < 1:
        raise ValueError(f"need 1 <= min_frames <= max_frames and num_lengths >= 1, got {lo}, {hi}, {n}")
    if n == 1 or lo == hi:
        return [hi]
    return [int(np.floor(lo * (hi / lo) ** (i / (n - 1)) + 0.5)) for i in range(n)]


class BankView:
    """Utterances of a bank: index arrays only (first row, length and dense speaker label per utterance, on the host). `storage` is
    the bank's (capacity, dim) tensor, or None for a view that is only planned with. The index of ktf_egs.h is built lazily with numpy
    (`index()`) and uploaded once (`device_arrays()`)."""

    def __init__(self, row0, lens, labels, speaker_ids, storage=None, utt_ids=None):
        self.row0 = np.asarray(row0, np.int64).reshape(-1)
        self.lens = np.asarray(lens, np.int32).reshape(-1)
        self.labels = np.asarray(labels, np.int32).reshape(-1)
        self.speaker_ids = list(speaker_ids)
        self.utt_ids = list(range(len(self.lens))) if utt_ids is None else list(utt_ids)
        self.storage = storage
        if not (len(self.row0) == len(self.lens) == len(self.labels) == len(self.utt_ids)):
            raise ValueError("row0, lens, labels and utt_ids have one entry per utterance")
        if len(self.labels) and (self.labels.min() < 0 or self.labels.max() >= len(self.speaker_ids)):
            raise ValueError("a label outside [0, number of speakers)")
        self._index = self._dev = None

    # ------------------------------------------------------------------ sizes
    @property
    def num_speakers(self):
        return len(self.speaker_ids)

    @property
    def num_utts(self):
        return len(self.lens)

    @property
    def num_frames(self):
        return int(self.lens.astype(np.int64).sum())

    @property
    def max_len(self):
        return int(self.lens.max()) if len(self.lens) else 0

    # ------------------------------------------------------------------ the index
    def index(self):
        """{"spk_order", "spk_off", "spk_utts", "spk_utt_len", "spk_max_len"}: int32 numpy arrays, as ktf_egs.h orders them."""
        if self._index is None:
            S, U = self.num_speakers, self.num_utts
            u = np.arange(U)
            by = np.lexsort((u, -self.lens.astype(np.int64), self.labels))            # speaker, then length descending, then index
            off = np.zeros(S + 1, np.int64)
            np.cumsum(np.bincount(self.labels, minlength=S), out=off[1:])
            longest = np.zeros(S, np.int64)
            np.maximum.at(longest, self.labels, self.lens)
            order = np.lexsort((np.arange(S), -longest))
            i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
            self._index = {"spk_order": i32(order), "spk_off": i32(off), "spk_utts": i32(by), "spk_utt_len": i32(self.lens[by]),
                           "spk_max_len": i32(longest)}
        return self._index

    def eligible_speakers(self, T):
        """n_spk of ktf_egs.h: the speakers whose longest utterance has at least T rows."""
        return int((self.index()["spk_max_len"] >= int(T)).sum())

    def device_arrays(self):
        """The view on the bank's device: row0 (int64), lens, labels and the four index arrays (int32) and their KtfEgsIndex."""
        if self.storage is None:
            raise L.KtfBackendError("this view has no bank on the GPU: it can be planned with on the host, not sampled")
        if self._dev is None:
            ix, dev = self.index(), self.storage.device
            up = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
            d = {k: up(ix[k]) for k in ("spk_order", "spk_off", "spk_utts", "spk_utt_len")}
            d.update(row0=up(self.row0), lens=up(self.lens), labels=up(self.labels))
            d["index"] = ops.egs_index(d["spk_order"], d["spk_off"], d["spk_utts"], d["spk_utt_len"])
            self._dev = d
        return self._dev

    # ------------------------------------------------------------------ the recipe's clean-up and the validation split
    def _subset(self, keep, speaker_ids=None, labels=None):
        keep = np.asarray(keep, np.int64)
        return BankView(self.row0[keep], self.lens[keep], self.labels[keep] if labels is None else labels,
                        self.speaker_ids if speaker_ids is None else speaker_ids, self.storage, [self.utt_ids[k] for k in keep])

    def filter(self, min_frames=400, min_utts_per_speaker=8):
        """The recipe's two clean-up steps, in this order: drop the utterances shorter than min_frames, then the speakers with fewer
        than min_utts_per_speaker left. The surviving speakers are renumbered densely (in label order); `speaker_ids` follows."""
        long_enough = self.lens >= int(min_frames)
        left = np.bincount(self.labels[long_enough], minlength=self.num_speakers)
        spk_keep = left >= max(int(min_utts_per_speaker), 1)
        keep = np.flatnonzero(long_enough & spk_keep[self.labels])
        new_label = np.cumsum(spk_keep) - 1
        return self._subset(keep, [s for s, k in zip(self.speaker_ids, spk_keep) if k], new_label[self.labels[keep]])

    def holdout(self, num_utts, seed):
        """(train_view, heldout_view) sharing storage and label numbering. Held-out utterance j is entry
        idx(philox((j, 0, 0, 2), seed)[0], n) of the n utterances, in view order, whose speaker still has at least two left for
        training: never a speaker's last one."""
        key = _words(seed)
        train, held = list(range(self.num_utts)), []
        left = np.bincount(self.labels, minlength=self.num_speakers)
        for j in range(int(num_utts)):
            cand = [u for u in train if left[self.labels[u]] >= 2]
            if not cand:
                raise ValueError(f"cannot hold out {num_utts} utterances: after {j} every speaker is down to its last one")
            u = cand[idx(ops.egs_philox((j & MASK32, 0, 0, HOLDOUT_STREAM), key)[0], len(cand))]
            train.remove(u)
            held.append(u)
            left[self.labels[u]] -= 1
        return self._subset(train), self._subset(sorted(held))


class FeatureBank(BankView):
    """(capacity_frames, dim) feature rows on the GPU, allocated once, filled by add() / add_wavs(). It is the view of all its
    utterances; filter() and holdout() give further views of the same storage."""

    def __init__(self, dim, capacity_frames, dtype=torch.float32, device=None):
        if dtype not in ops.EGS_DTYPES:
            raise ValueError(f"the bank stores torch.float32 or torch.float16, not {dtype}")
        if int(dim) < 1 or int(capacity_frames) < 1:
            raise ValueError("dim and capacity_frames are at least 1")
        L.require_gpu()
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise L.KtfBackendError("the bank lives on the GPU (no CPU fallback)")
        super().__init__([], [], [], [], torch.zeros((int(capacity_frames), int(dim)), dtype=dtype, device=device), [])
        self.dim, self.capacity_frames, self._used, self._label_of = int(dim), int(capacity_frames), 0, {}

    def add(self, feats, lens, speakers, utt_ids=None):
        """Appends the first lens[b] rows of each utterance of feats (B, T, dim) (fp32 / fp16 / bf16 on the bank's device). `speakers`:
        one hashable id per utterance, mapped to dense labels in first-seen order. Utterances of length 0 are skipped."""
        for t, what in ((feats, "feats"), (lens, "lens")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise L.KtfBackendError(f"{what} must be a tensor on the GPU (no CPU fallback)")
        if feats.dim() != 3 or feats.shape[2] != self.dim or feats.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"feats must be (B, T, {self.dim}) fp32 / fp16 / bf16, got {feats.dtype} {tuple(feats.shape)}")
        n = [int(v) for v in lens.cpu().reshape(-1)]
        speakers = list(speakers)
        utt_ids = [None] * len(n) if utt_ids is None else list(utt_ids)
        if not (len(n) == len(speakers) == len(utt_ids) == feats.shape[0]):
            raise ValueError("lens, speakers and utt_ids have one entry per utterance of feats")
        if any(v < 0 or v > feats.shape[1] for v in n):
            raise ValueError("a length outside [0, T]")
        if self._used + sum(n) > self.capacity_frames:
            raise ValueError(f"the bank holds {self.capacity_frames} frames: {self._used} used, {sum(n)} more do not fit")
        row0, lens_, labels, ids = [], [], [], []
        for b, v in enumerate(n):
            if v == 0:
                continue
            self.storage[self._used:self._used + v].copy_(feats[b, :v])
            if speakers[b] not in self._label_of:
                self._label_of[speakers[b]] = len(self.speaker_ids)
                self.speaker_ids.append(speakers[b])
            row0.append(self._used)
            lens_.append(v)
            labels.append(self._label_of[speakers[b]])
            ids.append(len(self.utt_ids) + len(ids) if utt_ids[b] is None else utt_ids[b])
            self._used += v
        self.row0 = np.concatenate([self.row0, np.asarray(row0, np.int64)])
        self.lens = np.concatenate([self.lens, np.asarray(lens_, np.int32)])
        self.labels = np.concatenate([self.labels, np.asarray(labels, np.int32)])
        self.utt_ids += ids
        self._index = self._dev = None
        return self

    def add_wavs(self, extractor, wavs, speakers):
        """add() of the CMVN'd, voiced-only rows XvectorExtractor.features gives for `wavs`."""
        return self.add(*extractor.features(wavs)[1:], speakers)


class ChunkSampler:
    """Iterator over (feats (B_local, T, dim) fp32, lens (B_local,) int32 all equal to T, labels (B_local,) int32): what
    `for feats, lens, labels in batches:` of a training loop consumes. Every chunk of a batch has one length, as in a Kaldi egs
    archive: entry idx(philox((0, step_lo, step_hi, 1), seed)[0], L) of length_table(min_frames, max_frames, num_lengths).
    `batch_size` is the global size; rank r of `world` gets the global rows r, r + world, ... The output buffers come from a
    two-deep ring owned by the sampler: A BATCH IS VALID UNTIL THE NEXT-BUT-ONE CALL of next() / batch() (clone what must live
    longer); the one call per step is ktf_egs_sample, on the current stream."""

    def __init__(self, bank, batch_size, min_frames=200, max_frames=400, num_lengths=5, seed=0, rank=0, world=1):
        self.lengths = length_table(min_frames, max_frames, num_lengths)
        if int(max_frames) > bank.max_len:
            raise ValueError(f"max_frames {max_frames} above the bank's longest utterance {bank.max_len}: no speaker is eligible")
        batch_size, rank, world = int(batch_size), int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside [0, world = {world})")
        if batch_size < 1 or batch_size % world:
            raise ValueError(f"world {world} does not divide the global batch size {batch_size}")
        _words(seed)
        self.bank, self.batch_size, self.seed, self.step, self.rank, self.world = bank, batch_size, int(seed), 0, rank, world
        self.local_size = batch_size // world
        self._ring, self._turn, self._lens = None, 0, {}

    def global_rows(self):
        """(b0, b_stride, B_local): this rank's rows of the global batch."""
        return self.rank, self.world, self.local_size

    def chunk_length(self, step):
        """T of `step`, on the host."""
        r0 = ops.egs_philox((0,) + _words(step) + (LENGTH_STREAM,), _words(self.seed))[0]
        return self.lengths[idx(r0, len(self.lengths))]

    def _buffers(self):
        d = self.bank.device_arrays()
        if self._ring is None:
            dev, B = self.bank.storage.device, self.local_size
            self._ring = [(torch.empty(B * max(self.lengths) * self.bank.storage.shape[1], dtype=torch.float32, device=dev),
                           torch.empty((3, B), dtype=torch.int32, device=dev)) for _ in range(2)]
        flat, plan = self._ring[self._turn]
        self._turn ^= 1
        return d, flat, plan

    def _lens_of(self, T, device):
        if T not in self._lens:
            self._lens[T] = torch.full((self.local_size,), T, dtype=torch.int32, device=device)
        return self._lens[T]

    def batch(self, step):
        d, flat, plan = self._buffers()
        T, B, D = self.chunk_length(step), self.local_size, self.bank.storage.shape[1]
        out = flat[:B * T * D].view(B, T, D)
        ops.egs_sample(d["index"], self.bank.num_speakers, self.bank.eligible_speakers(T), self.seed, step, T, self.rank, self.world,
                       self.bank.storage, d["row0"], d["lens"], out, plan[0], plan[1], plan[2])
        return out, self._lens_of(T, flat.device), plan[2]

    def plan(self, step):
        """(utt, offset, label) (B_local,) int32 of `step`, as owned tensors: the draw without the gather. utt indexes the view."""
        d = self.bank.device_arrays()
        utt, offset, label = torch.empty((3, self.local_size), dtype=torch.int32, device=self.bank.storage.device).unbind(0)
        T = self.chunk_length(step)
        return ops.egs_draw(d["index"], self.bank.num_speakers, self.bank.num_utts, self.bank.eligible_speakers(T), self.seed, step, T,
                            self.rank, self.world, utt, offset, label)

    def gather(self, utt, offset, T):
        """An explicit plan (validation sets, tests): (feats (B, T, dim), lens, labels) as owned tensors. A row the plan gets wrong
        (utt outside the view, a chunk outside its utterance) is zeros with label -1."""
        d = self.bank.device_arrays()
        dev = self.bank.storage.device
        utt = torch.as_tensor(utt, dtype=torch.int32, device=dev).contiguous()
        offset = torch.as_tensor(offset, dtype=torch.int32, device=dev).contiguous()
        if utt.dim() != 1 or utt.shape != offset.shape or int(T) < 1:
            raise ValueError("utt and offset are (B,) and T is at least 1")
        B, T = utt.numel(), int(T)
        out = torch.empty((B, T, self.bank.storage.shape[1]), dtype=torch.float32, device=dev)
        ops.egs_gather(self.bank.storage, d["row0"], d["lens"], utt, offset, T, out)
        inside = (utt >= 0) & (utt < self.bank.num_utts)
        u = utt.clamp(0, self.bank.num_utts - 1).long()
        ok = inside & (offset >= 0) & (offset.long() + T <= d["lens"][u])
        labels = torch.where(ok, d["labels"][u], torch.full_like(utt, -1))
        return out, torch.full((B,), T, dtype=torch.int32, device=dev), labels

    def __iter__(self):
        return self

    def __next__(self):
        b = self.batch(self.step)
        self.step += 1
        return b

    next = __next__

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state):
        _words(state["seed"]), _words(state["step"])
        self.seed, self.step = int(state["seed"]), int(state["step"])
