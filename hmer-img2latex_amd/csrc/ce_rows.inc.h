// Cross entropy with label smoothing, one workgroup per (b,t) row (included inside an anonymous namespace by
// train_decoder.hip -- i2l_ce_label_smooth_fwd_bwd -- and by train_risk.hip -- i2l_ce_weighted_fwd_bwd).
//   row_loss = keep * ((1-eps)*nll + eps*(-mean_v logp));
//   dlogits  = keep * (softmax - (1-eps)*onehot - eps/V)   [gradient of the SUM over rows; the mean's 1/count
//   is applied later so that data-parallel ranks can all-reduce un-normalised sums].
// WEIGHTED: token row i belongs to sequence i / steps, which brings its own smoothing eps = smooth[seq] and a coefficient
// that scales dlogits; row_loss and row_keep stay unweighted (the ordered sum applies the coefficient, and needs the
// unweighted parts too).  With every coefficient 1 and one smoothing value the two instantiations write the same bits:
// the only extra operation is a multiplication by 1.f.
#pragma once

struct CeSeq {
    const float* coef;      // [rows / steps]
    const float* smooth;    // [rows / steps]
    int steps;
};

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits,
                                                      const int32_t* __restrict__ targets, float* __restrict__ dlogits,
                                                      float* __restrict__ row_loss, float* __restrict__ row_keep, int V,
                                                      int pad_id, float eps, CeSeq q) {
    __shared__ float red[8];
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + row * V;
    const int tgt = targets[row];
    float coef = 1.f;
    if constexpr (WEIGHTED) {
        const size_t seq = row / (size_t)q.steps;
        eps = q.smooth[seq];
        coef = q.coef[seq];
    }
    float m = -INFINITY;
    for (int v = tid; v < V; v += 256) m = fmaxf(m, x[v]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f, sx = 0.f;
    for (int v = tid; v < V; v += 256) { s += expf(x[v] - m); sx += x[v]; }
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off, 64); sx += __shfl_xor(sx, off, 64); }
    if (lane == 0) { red[wave] = s; red[4 + wave] = sx; }
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    sx = (red[4] + red[5]) + (red[6] + red[7]);
    const float lse = m + logf(s);
    const bool keep = tgt != pad_id;
    const int tg = min(max(tgt, 0), V - 1);
    if (dlogits) {
        float* d = dlogits + row * V;
        const float base = eps / (float)V;
        // softmax as exp(x - max) / sum, not exp(x - lse): lse is rounded to ulp(|lse|), which at |logits| ~ 1e4 is 1e-3
        for (int v = tid; v < V; v += 256) {
            float g = expf(x[v] - m) / s - base - (v == tg ? (1.f - eps) : 0.f);
            if constexpr (WEIGHTED) g *= coef;
            d[v] = keep ? g : 0.f;
        }
    }
    if (tid == 0) {
        const float nll = lse - x[tg];
        const float smooth = lse - sx / (float)V;
        // eps == 0: no smoothing term, as in torch -- a -inf logit makes it +inf, and 0 * inf is NaN
        row_loss[row] = !keep ? 0.f : eps > 0.f ? (1.f - eps) * nll + eps * smooth : nll;
        row_keep[row] = keep ? 1.f : 0.f;
    }
}
