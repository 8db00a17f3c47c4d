/*
 * ktf_optim.h -- the optimiser step of training: SGD (momentum, Nesterov) or Adam over one flat arena of parameters, with gradient
 * clipping by global norm and Kaldi-style max-change limits on every segment's update and on the whole model's, on the GPU. Entry
 * points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold here too (INTEGRATION.md section 2q;
 * kernels: csrc/optim.hip).
 *
 * No Kaldi source was at hand when this was written: max-change here is the rule below, not a port of nnet3's. The rules of this
 * header are the contract; tests/_optim_ref.py restates them in numpy.
 *
 * Layout. p, g, m and v are fp32 arrays of `total` elements (the arenas: parameters, gradients, first and second state). A table of
 * n_seg segments KtfOptimSeg {begin, end, group, max_change} names the elements [begin, end) of one tensor: begin is a multiple of
 * KTF_OPTIM_SLOT_ELEMS, begin <= end <= total, and segment s + 1 begins at or after the end of segment s (ascending, no overlap;
 * begin == end is an empty segment). Elements outside every segment are padding: never read, never written, NaN allowed. The table
 * is given twice: `segs_host` is read and checked by every call, `segs_dev` is a device copy of the same table that the kernels read.
 * Each segment belongs to one of n_groups <= KTF_OPTIM_MAX_GROUPS groups KtfOptimGroup {lr, weight_decay}; the groups are read from
 * host memory at call time and travel as kernel arguments (a learning-rate schedule costs no upload and no synchronisation).
 *
 * All arithmetic is fp64 on the fp32 inputs, every operation rounded on its own (no fused multiply-add), every stored value rounded
 * once to fp32. mu = momentum, wd and lr those of the element's group.
 *   1. Clipping (clip_norm > 0). G = sqrt(sum g^2) over the elements of all segments, c = G > clip_norm ? clip_norm / G : 1 (which is
 *      min(1, clip_norm / G), and 1 for G = 0). Clipping off: c = 1, G is not computed and reported as 0.
 *   2. Gradient. ghat = c * g + wd * p, or ghat = c * g where `decoupled`.
 *   3. KTF_OPTIM_SGD. m' = mu * m + ghat (torch's rule with dampening 0, its first step included: m starts at 0);
 *      d = nesterov ? ghat + mu * m' : m'. With mu = 0: d = ghat, m is neither read nor written and may be NULL. v is not looked at.
 *   4. KTF_OPTIM_ADAM. m' = beta1 * m + (1 - beta1) * ghat, v' = beta2 * v + (1 - beta2) * (ghat * ghat),
 *      d = (m' / (1 - beta1^step)) / (sqrt(v') / sqrt(1 - beta2^step) + eps): torch.optim.Adam's operations. 1 - beta, beta^step
 *      (pow) and the square root of the second correction are evaluated once on the host in double.
 *   5. Decoupled weight decay: d = d + wd * p (after rule 3 or 4).
 *   6. Max-change (on when max_change_global > 0 or any segment's max_change > 0). Per segment s: N_s = lr * sqrt(sum_s d^2),
 *      sigma_s = (max_change_s > 0 and N_s > max_change_s) ? max_change_s / N_s : 1. N = sqrt(sum_s (sigma_s * N_s)^2),
 *      sigma = (max_change_global > 0 and N > max_change_global) ? max_change_global / N : 1. A scale is 1 where its limit is off
 *      or its norm is 0. Max-change off: every scale is 1, N is not computed and reported as 0.
 *   7. Update. a = (sigma * sigma_s) * lr, p <- (float)(p - a * d), from the unrounded fp64 d. SGD with mu != 0 stores
 *      m <- (float)((sigma * sigma_s) * m'): a limited step is not made up for by the following ones. Adam stores (float)m' and
 *      (float)v' unscaled.
 *   8. Sums. No floating-point atomics. Element i belongs to slot i / KTF_OPTIM_SLOT_ELEMS, one workgroup of 256 threads per slot.
 *      With i = slot * KTF_OPTIM_SLOT_ELEMS + 4 * (t + 256 * k) + j, thread t adds the squares of its elements in ascending (k, j),
 *      k < KTF_OPTIM_SLOT_ELEMS / 1024, j < 4, starting from +0 (elements outside the segment add nothing); the 64 lanes of a wave
 *      are added by a butterfly over the lane distances 32, 16, 8, 4, 2, 1 and the four waves as ((0 + 1) + 2) + 3. The slot's sum
 *      goes into a workspace entry of its own. One finalize workgroup gives every segment a wave: lane l adds the segment's slots
 *      l, l + 64, ... in ascending order and the 64 lanes are added by the same butterfly; one thread then adds the segments in
 *      ascending order (for N: the (sigma_s * N_s)^2). The same call twice gives the same bits.
 *   9. Access. A thread reads and writes its four neighbouring elements as 16 bytes where they lie inside the segment and p, g, m and
 *      v (those the call uses) are 16-byte aligned, element by element otherwise. The values are the same.
 *  10. Non-finite guard. If G, an N_s or N is NaN or +-Inf the call changes nothing: p, m and v keep their bits and the skipped flag
 *      of the statistics is 1 (the scales reported are then those of the formulas above evaluated on the non-finite norms). With
 *      neither limit on nothing is reduced and there is NO guard: a non-finite gradient goes into p.
 *  11. Launches. Neither limit: one (apply). Clipping adds a reduce over g and a finalize; max-change adds a reduce that
 *      recomputes d and stores nothing, and a finalize. Both: five, whatever n_seg.
 *  12. Statistics. `stats` (device, 5 + n_seg doubles, may be NULL) receives G, c, N, sigma, skipped (0 or 1), then sigma_s per
 *      segment. Nothing is copied to the host and nothing waits.
 *  13. Never a fault. What the kernels read from the device table is clamped (elements to [0, total], groups to [0, n_groups),
 *      slots to the workspace): a device table that is not the host table gives wrong values, not a bad access.
 *  14. Refused (KTF_EINVAL, before any launch, no GPU needed): a null p, g, segs_host, segs_dev, groups or workspace; a null m where
 *      mu != 0 or kind is ADAM, a null v for ADAM; n_seg < 0; total < 0 or total >= 2^40; a segment whose begin is negative or no
 *      multiple of KTF_OPTIM_SLOT_ELEMS, whose end is below its begin or above total, that begins before its predecessor ends,
 *      whose group is outside [0, n_groups) or whose max_change is negative or not finite; n_groups outside
 *      [1, KTF_OPTIM_MAX_GROUPS]; lr or weight_decay negative or not finite; SGD: mu outside [0, 1) or nesterov with mu = 0;
 *      ADAM: beta1 or beta2 outside [0, 1), eps <= 0 or not finite, step < 1; clip_norm or max_change_global negative or not
 *      finite; an unknown kind; a workspace below ktf_optim_workspace_bytes or not 256-byte aligned; any two of p, g, m, v
 *      overlapping.
 */
#ifndef KTF_OPTIM_H_
#define KTF_OPTIM_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_OPTIM_SLOT_ELEMS 4096   /* elements per slot of partial sums; every segment begins at a multiple of it */
#define KTF_OPTIM_MAX_GROUPS 8
#define KTF_OPTIM_SGD 0
#define KTF_OPTIM_ADAM 1

typedef struct KtfOptimSeg {
    int64_t begin, end;      /* elements [begin, end) of the arenas */
    int32_t group;           /* index into the groups */
    float max_change;        /* limit on lr * |d| of this segment, 0 = off (rule 6) */
} KtfOptimSeg;

typedef struct KtfOptimGroup {
    double lr, weight_decay;
} KtfOptimGroup;

/* KTF_OPTIM_SLOT_ELEMS, for callers that do not read the header. */
int64_t ktf_optim_slot_elems(void);

/* Bytes of the workspace a call takes: al256(max(ceil(total / KTF_OPTIM_SLOT_ELEMS), 1) * 8) for the slots plus
 * al256((5 + n_seg) * 8) for the norms and scales plus al256(max(n_seg, 1) * 8) for the segments' sums (al256: rounded up to a
 * multiple of 256). Never 0; a negative KTF_* code on bad arguments (total < 0, total >= 2^40, n_seg < 0). */
int64_t ktf_optim_workspace_bytes(int64_t total, int32_t n_seg);

/* Rules 1 - 14. */
int ktf_optim_step(float* p, const float* g, float* m, float* v, int64_t total, const KtfOptimSeg* segs_host,
                   const KtfOptimSeg* segs_dev, int32_t n_seg, const KtfOptimGroup* groups, int32_t n_groups, int32_t kind,
                   double momentum, int32_t nesterov, double beta1, double beta2, double eps, int64_t step, int32_t decoupled,
                   double clip_norm, double max_change_global, double* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
