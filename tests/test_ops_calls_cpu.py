"""The back-end wrappers of ops.py (plda_score .. ahc, diar_segments .. vbx_loglike), pinned on the CPU in the manner of
test_runner_launches_cpu.py: the native library is replaced by a recorder (the pure host `*_workspace_bytes` symbols still answer
from the real libktf_hip.so, and are written out with their result), each case calls one wrapper on small CPU tensors, and the
symbol called, every integer / float / struct argument, which tensor every pointer argument is (an argument of the wrapper by name,
`out[k]` of what it returns, `ws` for a byte workspace of its own, `tmp` for any other tensor of its own, `host` for a host array,
`null`) and the shape, strides and dtype of what the wrapper returns are compared with tests/golden/ops_calls.txt.

    python tests/test_ops_calls_cpu.py --write      # regenerate the golden file (only for a deliberate change of behaviour)
"""

import contextlib
import ctypes as C
import difflib
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
from _recorder import STREAM, Recorder  # noqa: E402
from test_runner_launches_cpu import EVERY_LAUNCH, HOST_HELPERS as RUNNER_HOST_HELPERS  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ops_calls.txt")
HOST_HELPERS = re.compile(r"ktf_\w+_workspace_bytes")
# Symbols this test does not have to reach: what the extraction path calls (the runner test pins those), the front-end / VAD / CMVN /
# pooling / tail / conversion entry points of ops.py above plda_score, and the library's own bookkeeping. No back-end symbol is here.
FRONT_END = {
    "ktf_num_frames", "ktf_num_frames_padded", "ktf_frontend_f32", "ktf_frontend_plan", "ktf_dct_f32", "ktf_vad_mask_f32", "ktf_vad_index",
    "ktf_cmvn_f32", "ktf_vad_cmvn", "ktf_vad_cmvn_plan", "ktf_cmvn_plan", "ktf_route_short", "ktf_tdnn_last_kernel", "ktf_split_bf16",
    "ktf_affine_act_f32", "ktf_activation_f32", "ktf_convert_pad", "ktf_stats_pool_windowed_f32", "ktf_xvec_post_f32",
    "ktf_xvec_tail_f32", "ktf_plda_f64", "ktf_plda_f32",
}
BOOKKEEPING = {"ktf_version", "ktf_last_error", "ktf_build_id", "ktf_clock_probe"}
EXEMPT = EVERY_LAUNCH | {n for n in L.PROTOTYPES if RUNNER_HOST_HELPERS.fullmatch(n)} | FRONT_END | BOOKKEEPING

WS = object()           # a case's `workspace=WS`: the wrapper gets a callback that allocates (the tensor is named "workspace")
SCRATCH = object()      # a case's `scratch=SCRATCH`: the same for `scratch(role, shape, dtype)` (the tensors are named by role)
F32, F64, I32 = torch.float32, torch.float64, torch.int32


def t(*shape, dt=F32):
    return torch.zeros(shape, dtype=dt)


def wide(rows, cols, dt=F32):
    """(rows, cols) as a column slice of a wider buffer: its row stride is cols + 3."""
    return torch.zeros((rows, cols + 3), dtype=dt)[:, 1:cols + 1]


def _x_forms(D=5, F=7):
    """The three forms of a 2-D frame matrix the `x.stride(0) if F else D` rule tells apart."""
    return (("", lambda: t(F, D), F), ("_strided", lambda: wide(F, D), F), ("_F0", lambda: t(0, D), 0))


def cases():
    """[(label, wrapper name, keyword arguments)]: tensors are named by their keyword in the record."""
    out = []
    add = lambda label, fn, **kw: out.append((label, fn, kw))  # noqa: E731
    vad = L.VadCfg(5.5, 0.5, 0.12, 2, 0)
    cmn = L.CmvnCfg(300, 0, 1, 0)
    for dt, tag in ((F32, "f32"), (F64, "f64")):
        add(f"plda_score_{tag}", "plda_score", test_tr=t(5, 4, dt=dt), enroll_tr=t(3, 4, dt=dt), psi=t(4, dt=dt))
        add(f"plda_transform_n_{tag}", "plda_transform_n", x=t(5, 4, dt=dt), A=t(4, 4, dt=dt), offset=t(4, dt=dt), psi=t(4, dt=dt),
            num_examples=t(5, dt=dt), normalize_length=True, simple_length_norm=False)
        add(f"plda_score_n_{tag}", "plda_score_n", test_tr=t(5, 4, dt=dt), enroll_tr=t(3, 4, dt=dt), psi=t(4, dt=dt),
            enroll_num_examples=t(3, dt=dt))
        for T, ws in ((6, None), (6, WS), (0, None), (0, WS)):
            add(f"plda_trials_{tag}_T{T}_{'ws' if ws else 'fresh'}", "plda_trials", test_tr=t(5, 4, dt=dt), enroll_tr=t(3, 4, dt=dt),
                psi=t(4, dt=dt), enroll_num_examples=t(3, dt=dt), pairs=t(T, 2, dt=I32), workspace=ws)
        for top_n in (None, 3, 1 << 40):
            add(f"topn_stats_{tag}_top{top_n}", "topn_stats", x=t(4, 9, dt=dt), top_n=top_n)
        add(f"topn_stats_{tag}_strided", "topn_stats", x=wide(4, 9, dt), top_n=3)
        add(f"topn_stats_{tag}_transposed", "topn_stats", x=t(9, 4, dt=dt).t(), top_n=3)          # forces .contiguous()
        add(f"topn_stats_{tag}_one_row", "topn_stats", x=wide(1, 9, dt), top_n=3)
        add(f"topn_stats_{tag}_one_row_transposed", "topn_stats", x=t(9, 2, dt=dt).t()[:1], top_n=None)  # forces .contiguous()
        add(f"topn_stats_{tag}_no_rows", "topn_stats", x=t(0, 9, dt=dt), top_n=3)
        for role, counts, top_n in ((0, None, None), (0, t(6, dt=dt), 3), (1, None, 3), (1, t(4, dt=dt), None)):
            add(f"plda_cohort_stats_{tag}_role{role}_{'counts' if counts is not None else 'nocounts'}_top{top_n}", "plda_cohort_stats",
                rows_tr=t(4, 8, dt=dt), cohort_tr=t(6, 8, dt=dt), psi=t(8, dt=dt), counts=counts, role=role, top_n=top_n,
                mean=t(4, dt=F64), std=t(4, dt=F64), workspace=t(4096, dt=torch.uint8))
        for energy in (None, 0.3):
            for scratch in (None, SCRATCH):
                add(f"plda_dense_{tag}_energy{energy}_{'scratch' if scratch else 'fresh'}", "plda_dense", x=t(7, 6, dt=dt),
                    lengths=[3, 4], target_energy=energy, A=t(6, 6, dt=dt), offset=t(6, dt=dt), psi=t(6, dt=dt), mean64=t(6, dt=F64),
                    Tinv64=t(6, 6, dt=F64), psi64=t(6, dt=F64), normalize_length=True, simple_length_norm=False, scratch=scratch)
        for mc in (None, [1, 2]):
            for scratch in (None, SCRATCH):
                add(f"ahc_{tag}_{'min' if mc else 'nomin'}_{'scratch' if scratch else 'fresh'}", "ahc", scores=t(25, dt=dt), lengths=[3, 4],
                    threshold=0.5, min_clusters=mc, max_spk_fraction=0.75, read_costs=mc is not None, scratch=scratch)
        add(f"train_mean_{tag}", "train_mean", y=t(9, 6, dt=dt), ws=t(512, dt=torch.uint8))
        for idx, center, weights in ((None, None, None), (t(4, dt=I32), None, None), (None, t(6, dt=F64), None),
                                     (t(4, dt=I32), t(6, dt=F64), t(4, dt=F64))):
            add(f"train_gram_{tag}_{'idx' if idx is not None else 'all'}_{'c' if center is not None else 'noc'}_"
                f"{'w' if weights is not None else 'now'}", "train_gram", y=t(9, 6, dt=dt), ws=t(512, dt=torch.uint8), idx=idx, center=center,
                weights=weights)
    add("plda_cohort_workspace_bytes", "plda_cohort_workspace_bytes", R=4, Cn=6, dim=8, dtype_bytes=4)
    add("plda_dense_workspace_bytes", "plda_dense_workspace_bytes", lengths=[3, 4], dim=6, target_energy=None)
    add("plda_dense_workspace_bytes_energy", "plda_dense_workspace_bytes", lengths=[3, 4], dim=6, target_energy=0.3)
    add("ahc_workspace_bytes", "ahc_workspace_bytes", lengths=[3, 4], dtype_bytes=8)
    add("spk_mean", "spk_mean", raw=t(6, 4), offsets=t(4, dt=I32), utts=t(6, dt=I32), S=3)
    add("spk_mean_given", "spk_mean", raw=t(6, 4), offsets=t(4, dt=I32), utts=t(6, dt=I32), S=3, means=t(3, 4), num_utts=t(3, dt=I32))
    # sliding-window diarization front end
    fr = [30, 50]
    add("diar_segments", "diar_segments", mfcc=t(80, 5), frames=fr, offsets=t(3, dt=I32), vad_cfg=vad, seg_work=t(160, dt=I32),
        counts=t(4, dt=I32))
    add("diar_windows", "diar_windows", seg_work=t(160, dt=I32), frames=fr, offsets=t(3, dt=I32), W=15, P=7, M=5,
        win_work=t(160, dt=I32), counts=t(4, dt=I32))
    add("diar_compact", "diar_compact", seg_work=t(160, dt=I32), win_work=t(160, dt=I32), counts=t(4, dt=I32), frames=fr,
        offsets=t(3, dt=I32), G=3, S=9)
    add("diar_segment_cmn", "diar_segment_cmn", mfcc=t(80, 5), frames=fr, offsets=t(3, dt=I32), segments=t(3, 3, dt=I32), cmvn_cfg=cmn,
        out=t(80, 5), work=t(64))
    for odt, tag in ((F32, "f32"), (torch.bfloat16, "bf16")):
        add(f"diar_gather_{tag}", "diar_gather", cmn=t(80, 5), D=5, frames=fr, offsets=t(3, dt=I32), windows=t(9, 3, dt=I32), w0=2, n=4,
            out=t(4, 15, 32, dt=odt), lens=t(4, dt=I32))
    # i-vectors, full-covariance posteriors, GMM statistics, VB: every wrapper with the `x.stride(0) if F else D` rule in its three forms
    D, I, n, S, K = 5, 4, 3, 6, 2
    add("ivector_workspace_bytes", "ivector_workspace_bytes", B=2, I=I, D=D, S=S)
    add("ivector_train_workspace_bytes", "ivector_train_workspace_bytes", B=2, I=I, D=D, S=S)
    add("fgmm_workspace_bytes", "fgmm_workspace_bytes", F=7, I=I, D=D, n=n)
    add("gmm_post_dense_workspace_bytes", "gmm_post_dense_workspace_bytes", F=7, I=I)
    add("gmm_acc_workspace_bytes_diag", "gmm_acc_workspace_bytes", F=7, I=I, D=D, n=n, full=False)
    add("gmm_acc_workspace_bytes_full", "gmm_acc_workspace_bytes", F=7, I=I, D=D, n=n, full=True)
    add("vb_post_workspace_bytes", "vb_post_workspace_bytes", F=7, I=I)
    P = S * (S + 1) // 2
    for form, x, F in _x_forms(D):
        B = 2
        add(f"ivector_post{form}", "ivector_post", x=x(), W=t(2 * D, I), gconst=t(I), num_gselect=n, min_post=0.025)
        for dt, tag in ((F32, "f32"), (F64, "f64")):
            add(f"ivector_extract{form}_{tag}", "ivector_extract", x=x(), offsets=t(B + 1, dt=I32), gauss=t(F, n, dt=I32), post=t(F, n),
                posterior_scale=1.0, acoustic_weight=0.5, max_count=100.0, sigma_inv_M=t(I * D, S), U=t(I, P), prior_offset=10.0, dtype=dt)
        add(f"ivector_acc_stats{form}", "ivector_acc_stats", x=x(), offsets=t(B + 1, dt=I32), gauss=t(F, n, dt=I32), post=t(F, n),
            posterior_scale=1.0, sigma_inv_M=t(I * D, S), U=t(I, P), prior_offset=10.0, gamma=t(I, dt=F64), Y=t(I * D, S, dt=F64),
            R=t(I, P, dt=F64), ivector_sum=t(S, dt=F64), ivector_scatter=t(P, dt=F64), totals=t(2, dt=F64))
        add(f"ivector_acc_second_order{form}", "ivector_acc_second_order", x=x(), gauss=t(F, n, dt=I32), post=t(F, n), posterior_scale=0.5,
            Ssec=t(I, D, D, dt=F64))
        add(f"fgmm_post{form}", "fgmm_post", x=x(), gselect=t(F, n, dt=I32), means_invcovars=t(I, D), inv_covars=t(I, D, D), gconst=t(I),
            min_post=0.025)
        for want in (True, False):
            add(f"fgmm_post_ll{form}_{'ll' if want else 'noll'}", "fgmm_post_ll", x=x(), gselect=t(F, n, dt=I32), means_invcovars=t(I, D),
                inv_covars=t(I, D, D), gconst=t(I), min_post=0.025, want_loglike=want)
        for valid in (None, t(1, dt=I32)):
            add(f"gmm_post_preselect{form}_{'valid' if valid is not None else 'novalid'}", "gmm_post_preselect", x=x(),
                gselect=t(F, n, dt=I32), means_invvars=t(I, D), inv_vars=t(I, D), gconst=t(I), valid=valid)
        add(f"gmm_post_dense{form}", "gmm_post_dense", x=x(), W=t(2 * D, I), gconst=t(I))
        for full in (False, True):
            add(f"gmm_acc{form}_{'full' if full else 'diag'}", "gmm_acc", x=x(), gauss=t(F, n, dt=I32), post=t(F, n), occ=t(I, dt=F64),
                mean_acc=t(I, D, dt=F64), second_acc=t(I, D, D, dt=F64) if full else t(I, D, dt=F64))
        add(f"vb_post{form}", "vb_post", x=x(), W=t(2 * D, I), gconst=t(I), num_slots=n, ll_scale=1.0, stat_scale=0.2, sparsity_thr=0.001,
            truncated=t(1, dt=I32))
        TB = 4 if F else 0
        add(f"vb_speaker_stats{form}", "vb_speaker_stats", x=x(), offsets=t(B + 1, dt=I32), boffsets=t(B + 1, dt=I32), downsample=2,
            post=t(F, n), start=t(I + 1, dt=I32), pairs=t(F * n, dt=I32), means=t(I, D, dt=F64), q=t(TB, K, dt=F64))
        add(f"vb_block_loglike{form}", "vb_block_loglike", x=x(), offsets=t(B + 1, dt=I32), boffsets=t(B + 1, dt=I32), downsample=2, TB=TB,
            gauss=t(F, n, dt=I32), post=t(F, n), means=t(I, D, dt=F64), h=t(B * K, I * D, dt=F64), g=t(B * K, I, dt=F64), K=K)
    add("atb_f64", "atb_f64", A=t(7, 3, dt=F64), B=t(7, 4, dt=F64), C=t(3, 4, dt=F64))
    add("atb_f64_strided", "atb_f64", A=wide(7, 3, F64), B=wide(7, 4, F64), C=wide(3, 4, F64))
    add("atb_f64_K0", "atb_f64", A=t(0, 3, dt=F64), B=t(0, 4, dt=F64), C=t(3, 4, dt=F64))
    for lengths in (None, t(2, dt=I32)):
        add(f"add_deltas_{'lens' if lengths is not None else 'nolens'}", "add_deltas", x=t(2, 9, 5), lengths=lengths, coeffs=t(3, 9),
            order=2, window=2)
    add("add_deltas_strided", "add_deltas", x=torch.zeros((2, 9, 8))[:, :, :5], lengths=None, coeffs=t(3, 9), order=2, window=2)
    add("add_deltas_B1", "add_deltas", x=torch.zeros((1, 9, 8))[:, :, :5], lengths=None, coeffs=t(3, 9), order=2, window=2)
    add("add_deltas_T1", "add_deltas", x=torch.zeros((2, 1, 8))[:, :, :5], lengths=None, coeffs=t(3, 9), order=2, window=2)
    # back-end training
    add("train_workspace", "train_workspace", rows=9, D=6, device="cpu")
    add("train_class_means", "train_class_means", x=t(9, 6), offsets=t(4, dt=I32), utts=t(9, dt=I32), S=3)
    add("plda_em_project", "plda_em_project", mu=t(3, 6, dt=F64), mbar=t(6, dt=F64), P=t(6, 6, dt=F64), lam=t(6, dt=F64),
        counts=t(3, dt=I32))
    # VB-HMM resegmentation and VBx
    add("vb_bucket", "vb_bucket", gauss=t(7, n, dt=I32), I=I)
    add("vb_speaker_update", "vb_speaker_update", Nst=t(4, I, dt=F64), Fst=t(4, I * D, dt=F64), Bm=t(I * D, 3, dt=F64), U=t(I, 6, dt=F64))
    for fn in ("vb_forward_backward", "vb_forward_backward_serial"):
        add(fn, fn, lls=t(4, K, dt=F64), boffsets=t(3, dt=I32), sp=t(2, K, dt=F64), loop_prob=0.9)
    add("vb_loglike_sums", "vb_loglike_sums", loglike=t(7), offsets=t(3, dt=I32))
    add("vb_bound", "vb_bound", gsum=t(2, dt=F64), tll=t(2, dt=F64), kl=t(4, dt=F64), stat_scale=0.2)
    add("vbx_prepare", "vbx_prepare", x=t(7, 6, dt=F64), phi=t(6, dt=F64))
    add("vbx_speaker_update", "vbx_speaker_update", gamma=t(7, K, dt=F64), rho=t(7, 6, dt=F64), phi=t(6, dt=F64), fa_over_fb=0.3 / 17.0,
        offsets=t(3, dt=I32))
    add("vbx_loglike", "vbx_loglike", rho=t(7, 6, dt=F64), G=t(7, dt=F64), alpha=t(2, K, 6, dt=F64), c=t(2, K, dt=F64), Fa=0.3,
        offsets=t(3, dt=I32))
    return out


# ----------------------------------------------------------------------------- recorder
class _Ptr(C.c_void_p):
    """What the test makes L.ptr return: the pointer, and the tensor it came from."""


class _OpsRecorder(Recorder):
    def __init__(self, real):
        super().__init__(real, HOST_HELPERS, names=lambda addr: "host", log_host=True)
        self.seen = []          # the tensors of the pointer arguments, in order: a line holds "@k@" until `resolve` names them

    def ptr(self, tensor):
        if tensor is None:
            return None
        p = _Ptr(tensor.data_ptr())
        p.tensor = tensor
        return p

    def arg(self, a):
        if isinstance(a, _Ptr):
            self.seen.append(a.tensor)
            return f"@{len(self.seen) - 1}@"
        return super().arg(a)

    def resolve(self, named, outs):
        def same(a, b):
            """b is a, or a view into a's memory: -> the byte offset, else None."""
            if a is b:
                return 0
            if a.numel() and b.numel() and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr():
                return b.data_ptr() - a.data_ptr()
            return None

        def name(k):
            tensor = self.seen[k]
            for tag, cand in list(named.items()) + [(f"out[{i}]", o) for i, o in enumerate(outs)]:
                off = same(cand, tensor) if isinstance(cand, torch.Tensor) else None
                if off is not None:
                    return tag + (f"+{off}" if off else "")
            if tensor.dtype == torch.uint8 and tensor.dim() == 1:
                return "ws"
            return f"tmp{list(tensor.shape)}{str(tensor.dtype)[6:]}"
        names = [name(k) for k in range(len(self.seen))]
        self.lines = [re.sub(r"@(\d+)@", lambda m: names[int(m.group(1))], line) for line in self.lines]


def _flat(res):
    if isinstance(res, (tuple, list)):
        return [o for r in res for o in _flat(r)]
    return [res]


def _show(v):
    if isinstance(v, torch.Tensor):
        return f"{list(v.shape)}{list(v.stride())}{str(v.dtype)[6:]}"
    if isinstance(v, C.Structure):
        return type(v).__name__
    return "WS" if v is WS else "SCRATCH" if v is SCRATCH else repr(v)


def run_case(monkeypatch, case):
    label, fn, kw = case
    rec = _OpsRecorder(L.load())
    named = {k: v for k, v in kw.items() if isinstance(v, torch.Tensor)}
    args = dict(kw)
    if kw.get("workspace") is WS:
        args["workspace"] = lambda nbytes: named.setdefault("workspace", torch.empty((nbytes,), dtype=torch.uint8))
    if kw.get("scratch") is SCRATCH:
        args["scratch"] = lambda role, shape, dtype: named.setdefault(role, torch.empty(shape, dtype=dtype))
    with monkeypatch.context() as m:
        m.setattr(L, "_lib", rec)
        m.setattr(L, "load", lambda: rec)
        m.setattr(L, "require_gpu", lambda: None)
        m.setattr(L, "stream_ptr", lambda: STREAM)
        m.setattr(L, "on_device", lambda device: contextlib.nullcontext())
        m.setattr(L, "ptr", rec.ptr)
        res = getattr(ops, fn)(**args)
    outs = _flat(res)
    rec.resolve(named, [o for o in outs if isinstance(o, torch.Tensor)])
    k, shown = 0, []
    for o in outs:
        if isinstance(o, torch.Tensor):
            given = next((tag for tag, cand in named.items() if cand is o), None)
            shown.append(f"{given or f'out[{k}]'}={_show(o)}")
            k += 1
        else:
            shown.append(repr(o))
    head = f"== {label}: {fn}({', '.join(f'{k}={_show(v)}' for k, v in kw.items())})"
    return [head] + rec.lines + ["-> " + ", ".join(shown)], rec.called


def record(monkeypatch):
    lines, called = [], set()
    for case in cases():
        ls, c = run_case(monkeypatch, case)
        lines += ls
        called |= c
    return lines, called


def missing(called):
    return sorted(set(L.PROTOTYPES) - EXEMPT - called)


def test_no_backend_symbol_is_exempt():
    backend = re.compile(r"ktf_(plda_(score|transform_n|trials|cohort|dense|em)|spk_mean|topn|ahc|diar|ivector|atb|fgmm|gmm|add_deltas|train|vb_|vbx_)")
    assert not [n for n in EXEMPT if backend.match(n)]


def test_ops_calls_match_golden(monkeypatch):
    lines, called = record(monkeypatch)
    assert not missing(called), f"the cases do not reach {missing(called)}"
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    if lines != want:
        diff = list(difflib.unified_diff(want, lines, "golden", "ops", lineterm="", n=2))
        raise AssertionError("the back-end wrappers' library calls changed:\n" + "\n".join(diff[:80]))


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    mp = __import__("pytest").MonkeyPatch()
    try:
        lines, called = record(mp)
    finally:
        mp.undo()
    if missing(called):
        sys.exit(f"the cases do not reach {missing(called)}")
    with open(GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{GOLDEN}: {len(lines)} lines, {len(cases())} cases")
