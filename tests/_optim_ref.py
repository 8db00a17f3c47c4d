"""The optimiser step of include/ktf_optim.h in numpy fp64, rounding to fp32 exactly where the header rounds (its rule numbers in
the comments). `step` returns the new arrays, the norms and scales of the statistics, and the magnitudes the GPU tests bound their
errors with. sums="kernel" adds in the order of rule 8 (the kernels' bits); sums="exact" adds every sum exactly and rounds it once
(math.fsum): the reference of the tests on Gaussian inputs."""

import math

import numpy as np

SLOT = 4096          # KTF_OPTIM_SLOT_ELEMS
THREADS = 256
SGD, ADAM = "sgd", "adam"


def layout(sizes, slot=SLOT):
    """(begin, end) of tensors of `sizes` elements laid out one after the other on slot boundaries, and the arena's length."""
    rows, cursor = [], 0
    for n in sizes:
        rows.append((cursor, cursor + n))
        cursor = -(-(cursor + n) // slot) * slot
    return rows, max(cursor, slot)


def _segment_sum(sq, begin, end, sums):
    """The sum of sq[begin:end] (begin on a slot boundary) as rule 8 adds it, or exactly."""
    if sums == "exact":
        return math.fsum(sq[begin:end].tolist())
    lanes = np.zeros(64)                                                    # the finalize wave: lane l adds the slots l, l + 64, ...
    for index, s0 in enumerate(range(begin, end, SLOT)):
        chunk = np.zeros(SLOT)
        n = min(end, s0 + SLOT) - s0
        chunk[:n] = sq[s0:s0 + n]
        quads = chunk.reshape(SLOT // (4 * THREADS), THREADS, 4)          # [k][t][j]
        lane = np.zeros(THREADS)
        for k in range(quads.shape[0]):
            for j in range(4):
                lane = lane + quads[k, :, j]
        wave = lane.reshape(THREADS // 64, 64)
        for off in (32, 16, 8, 4, 2, 1):
            wave = wave + wave[:, np.arange(64) ^ off]
        slot_sum = ((wave[0, 0] + wave[1, 0]) + wave[2, 0]) + wave[3, 0]
        lanes[index % 64] = lanes[index % 64] + slot_sum
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ off]
    return float(lanes[0])


def _scale(limit, norm):
    """limit / norm where the limit is on and the norm above it, 1 otherwise (NaN included)."""
    return limit / norm if (limit > 0.0 and norm > limit) else 1.0


def step(p, g, m, v, segs, groups, kind=SGD, momentum=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8, step=1, decoupled=False,
         clip_norm=0.0, max_change_global=0.0, sums="kernel", dtype=np.float32):
    """p, g, m, v: float32 arrays of the arena's length (m, v may be None where the rule does not use them); segs: rows
    (begin, end, group, max_change); groups: rows (lr, weight_decay). Elements outside the segments are carried over untouched.
    dtype: what the arrays hold and stored values are rounded to; np.float64 leaves the rule itself, for checking it against torch."""
    f32 = dtype
    p = np.asarray(p, dtype=f32)
    g = np.asarray(g, dtype=f32)
    has_m = kind == ADAM or momentum != 0.0
    new_p = p.copy()
    new_m = None if m is None else np.asarray(m, dtype=f32).copy()
    new_v = None if v is None else np.asarray(v, dtype=f32).copy()
    has_clip = clip_norm > 0.0
    has_change = max_change_global > 0.0 or any(float(np.float32(s[3])) > 0.0 for s in segs)
    out = dict(G=0.0, c=1.0, N=0.0, sigma=1.0, skipped=0.0, sigma_s=np.ones(len(segs)), n_terms=sum(e - b for b, e, _, _ in segs))

    with np.errstate(all="ignore"):
        if has_clip:                                                        # rule 1
            parts = [_segment_sum(g.astype(np.float64) ** 2, b, e, sums) for b, e, _, _ in segs]
            total = math.fsum(parts) if sums == "exact" else float(np.add.accumulate(np.array([0.0] + parts))[-1])
            out["G"] = float(np.sqrt(np.float64(total)))
            out["c"] = _scale(clip_norm, out["G"])
            if not np.isfinite(out["G"]):
                out["skipped"] = 1.0
        c = out["c"]
        if kind == ADAM:
            b1, b2 = float(betas[0]), float(betas[1])
            om1, om2 = 1.0 - b1, 1.0 - b2
            bc1 = 1.0 - math.pow(b1, float(step))
            bc2_sqrt = math.sqrt(1.0 - math.pow(b2, float(step)))

        per = []
        for b, e, grp, _ in segs:
            lr, wd = (float(x) for x in groups[grp])
            P, Gd = p[b:e].astype(np.float64), g[b:e].astype(np.float64)
            gh = c * Gd                                                      # rule 2
            gh_mag = np.abs(gh)
            if not decoupled:
                gh = gh + wd * P
                gh_mag = gh_mag + np.abs(wd * P)
            m1 = v1 = None
            if kind == SGD:                                                  # rule 3
                if has_m:
                    M = new_m[b:e].astype(np.float64)
                    m1 = momentum * M + gh
                    m_mag = np.abs(momentum * M) + gh_mag
                    d = gh + momentum * m1 if nesterov else m1
                    sens = (1.0 + momentum) if nesterov else 1.0           # |dd / dghat|
                else:
                    d, m_mag, sens = gh, None, 1.0
                sens = sens * np.abs(c * Gd)
                v_mag = None
            else:                                                            # rule 4
                M, V = new_m[b:e].astype(np.float64), new_v[b:e].astype(np.float64)
                m1 = b1 * M + om1 * gh
                v1 = b2 * V + om2 * (gh * gh)
                m_mag = np.abs(b1 * M) + om1 * gh_mag
                v_mag = np.abs(b2 * V) + om2 * (gh_mag * gh_mag)
                root = np.sqrt(v1)
                den = root / bc2_sqrt + eps
                d = (m1 / bc1) / den
                droot = np.where(root > 0.0, om2 * np.abs(gh) / np.where(root > 0.0, root, 1.0), 0.0) / bc2_sqrt   # |d den / d ghat|
                sens = (om1 / bc1 / den + np.abs(m1 / bc1) * droot / (den * den)) * np.abs(c * Gd)
            if decoupled:                                                    # rule 5
                d = d + wd * P
            per.append(dict(lr=lr, P=P, d=d, m1=m1, v1=v1, m_mag=m_mag, v_mag=v_mag, sens=sens))

        Ns = np.zeros(len(segs))
        Ns_sens = np.zeros(len(segs))
        if has_change:                                                       # rule 6
            parts = []
            for i, ((b, e, _, mc), s) in enumerate(zip(segs, per)):
                dd = np.zeros(len(p))
                dd[b:e] = s["d"] * s["d"]
                Ns[i] = s["lr"] * float(np.sqrt(np.float64(_segment_sum(dd, b, e, sums))))
                Ns_sens[i] = s["lr"] * math.sqrt(math.fsum((s["sens"] ** 2).tolist())) if np.isfinite(s["sens"]).all() else np.inf
                out["sigma_s"][i] = _scale(float(np.float32(mc)), Ns[i])
                t = out["sigma_s"][i] * Ns[i]
                parts.append(float(t * t))
                if not np.isfinite(Ns[i]):
                    out["skipped"] = 1.0
            total = math.fsum(parts) if sums == "exact" else float(np.add.accumulate(np.array([0.0] + parts))[-1])
            out["N"] = float(np.sqrt(np.float64(total)))
            out["sigma"] = _scale(max_change_global, out["N"])
            if not np.isfinite(out["N"]):
                out["skipped"] = 1.0
        out["Ns"], out["Ns_sens"] = Ns, Ns_sens

        p_mag = np.zeros(len(p))
        m_mag = np.zeros(len(p))
        v_mag = np.zeros(len(p))
        if not out["skipped"]:                                               # rule 7 (rule 10 otherwise)
            for i, ((b, e, _, _), s) in enumerate(zip(segs, per)):
                scale = out["sigma"] * out["sigma_s"][i] if has_change else 1.0
                a = scale * s["lr"]
                new_p[b:e] = (s["P"] - a * s["d"]).astype(f32)
                p_mag[b:e] = np.abs(s["P"]) + np.abs(a * s["d"])          # |p| + |step|
                if kind == SGD and has_m:
                    new_m[b:e] = (scale * s["m1"]).astype(f32)
                    m_mag[b:e] = scale * s["m_mag"]
                elif kind == ADAM:
                    new_m[b:e] = s["m1"].astype(f32)
                    new_v[b:e] = s["v1"].astype(f32)
                    m_mag[b:e], v_mag[b:e] = s["m_mag"], s["v_mag"]
    out.update(p=new_p, m=new_m, v=new_v, p_mag=p_mag, m_mag=m_mag, v_mag=v_mag)
    return out


def stats_vector(out):
    """The statistics of rule 12 as the kernels lay them out."""
    return np.concatenate([[out["G"], out["c"], out["N"], out["sigma"], out["skipped"]], out["sigma_s"]])
