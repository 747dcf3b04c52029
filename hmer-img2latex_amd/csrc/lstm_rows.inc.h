// Row-kernel building blocks shared by inference (decode.hip) and training (train_decoder.hip): the gate functions, the
// software-pipelined fmaf matvec and the butterfly wave reductions (also attention.hip).  Inference and training agree
// bit for bit on the gate math because both use this one copy.
// Included inside each translation unit's anonymous namespace.
#pragma once

// Gate functions of the search and training kernels: hardware exp2 / reciprocal (v_exp_f32, v_rcp_f32: ~1 ulp each)
// instead of libm's expf / tanhf and an IEEE division -- the LSTM cell is a chain of five of them on the critical path
// of every step (~150 dependent instructions -> ~30).  Absolute error <= ~2e-7 per call, the class of the vectorised
// expf / tanhf ATen itself uses; saturation: exp -> inf gives 1/inf = 0, exp -> 0 gives -1 / 0+.
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * x) + 1.f); }

// acc[r] += sum_k W[k][0..3] * x[r][k], k ascending (one fmaf chain per output).
// The weight stream is software-pipelined: while the FMAs of one batch of PF rows run, the
// loads of the next batch are already in flight (two register sets, counted vmcnt by the
// compiler), so one wave per SIMD keeps ~PF 16-byte loads per lane outstanding.
constexpr int PF = 8;

template <int R>
__device__ __forceinline__ void fma_rows(float4 (&acc)[R], const float4 (&w)[PF], const float* xs, int xstride, int k) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int i4 = 0; i4 < PF; i4 += 4) {
            const float4 xa = *reinterpret_cast<const float4*>(xs + r * xstride + k + i4);
            const float xv[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[r].x = fmaf(w[i4 + i].x, xv[i], acc[r].x);
                acc[r].y = fmaf(w[i4 + i].y, xv[i], acc[r].y);
                acc[r].z = fmaf(w[i4 + i].z, xv[i], acc[r].z);
                acc[r].w = fmaf(w[i4 + i].w, xv[i], acc[r].w);
            }
        }
    }
}

template <typename VT>
__device__ __forceinline__ void load_batch(VT (&w)[PF], const float* __restrict__ Wcol, size_t ldw) {
#pragma unroll
    for (int i = 0; i < PF; ++i) w[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)i * ldw);
}

// matvec whose first batch (rows 0..PF-1) was loaded earlier by load_batch (prefetch across a barrier).
template <int R, typename VT>
__device__ __forceinline__ void matvec_pre(VT (&acc)[R], VT (&wa)[PF], const float* __restrict__ Wcol, size_t ldw,
                                           const float* xs, int xstride, int H) {
    VT wb[PF];
    int k = 0;
    for (; k + 2 * PF < H; k += 2 * PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) wb[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)(k + PF + i) * ldw);
        __builtin_amdgcn_sched_barrier(0);
        fma_rows<R>(acc, wa, xs, xstride, k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < PF; ++i) wa[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)(k + 2 * PF + i) * ldw);
        __builtin_amdgcn_sched_barrier(0);
        fma_rows<R>(acc, wb, xs, xstride, k + PF);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) wb[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)(k + PF + i) * ldw);
    __builtin_amdgcn_sched_barrier(0);
    fma_rows<R>(acc, wa, xs, xstride, k);
    fma_rows<R>(acc, wb, xs, xstride, k + PF);
}

// acc[r] += sum_{k<H} W[k][0..3] * xs[r*xstride + k];  H % (2*PF) == 0.
template <int R, typename VT>
__device__ __forceinline__ void matvec(VT (&acc)[R], const float* __restrict__ Wcol, size_t ldw, const float* xs,
                                       int xstride, int H) {
    VT wa[PF], wb[PF];
    // No load sits under a condition: the compiler can then count outstanding loads exactly
    // (s_waitcnt vmcnt(PF) before a batch is used) instead of draining to vmcnt(0) at a join.
#pragma unroll
    for (int i = 0; i < PF; ++i) wa[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)i * ldw);
    int k = 0;
    for (; k + 2 * PF < H; k += 2 * PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) wb[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)(k + PF + i) * ldw);
        __builtin_amdgcn_sched_barrier(0);                // keep the batch of loads ahead of the FMAs
        fma_rows<R>(acc, wa, xs, xstride, k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < PF; ++i) wa[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)(k + 2 * PF + i) * ldw);
        __builtin_amdgcn_sched_barrier(0);
        fma_rows<R>(acc, wb, xs, xstride, k + PF);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) wb[i] = *reinterpret_cast<const VT*>(Wcol + (size_t)(k + PF + i) * ldw);
    __builtin_amdgcn_sched_barrier(0);
    fma_rows<R>(acc, wa, xs, xstride, k);
    fma_rows<R>(acc, wb, xs, xstride, k + PF);
}

// butterfly reductions over the 64 lanes of a wave (every lane gets the result)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// (value, index) max with "first index wins" over the 64 lanes of a wave.
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}
