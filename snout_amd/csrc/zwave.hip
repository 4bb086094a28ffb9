// zwave.hip — Z-Wave (ITU-T G.9959, R2: 40 kbit/s 2-FSK) receive kernels for gfx950 (CDNA4, wave64).
//
// Replaces the GNU Radio flowgraph of the reference (snout/modulations/ZWave/hackrf/ZWave_rx/top_block.py:41-90),
// input IQ at 800 ksps tuned to channel + 200 kHz (the signal sits at -200 kHz):
//   z1 freq_xlating_fir_filter_ccc(1, 39 taps, -200e3, 800e3)  \
//   z2 simple_squelch_cc(-40, 1)                                |  zw_front  (fused, one f32 out per sample)
//   z3 quadrature_demod_cf(2 fs / (2 pi 20e3 / 8))              |
//   z4 fir_filter_fff(1, 193 taps)                             /
//   z5 clock_recovery_mm_ff(20, 0.25 0.175^2, 0.5, 0.175, 0.005) \
//   z6 binary_slicer_fb                                          |  zw_lanes  (one thread per lane)
//   z7 Zwave.packet_sink (restated from G.9959)      /
//   ordered records                                                 zw_scan + zw_copy
//
// Arithmetic order (tests/zwave_ref.py states the same, bit for bit; -ffp-contract=off):
//   z1  u[m] = j^m x[m] (exact sign / swap, x[m < 0] = 0);  y[n] = sum_{k=0..38} h1[k] u[n-k] on the real and the
//       imaginary part apart, acc = 0, acc = acc + h1[k] * v in tap order (= j^n sum h1[k] (-j)^k x[n-k]; the two
//       forms round alike up to the sign of a zero, which nothing downstream can see)
//   z2  p = re re + im im;  y[n] if (double)p >= 1e-4, else 0
//   z3  d[n] = g * fast_atan2f(Im(y[n] conj y[n-1]), Re(...)) (zb_discrim.h), y[-1] = 0, g = (float)(1.6e6 / (2 pi 2.5e3))
//   z4  f[n] = sum_{k=0..192} h2[k] d[n-k], acc = 0, acc = acc + h2[k] * d in tap order, d[n < 0] = 0
//   z5  GNU Radio 3.7 M&M with the 802.15.4 path's MMSE bank and fma chain (zigbee.hip zb_mm)
#include "common.h"
#include "zb_discrim.h"
#include "iq_fmt.h"
#include "zwave_taps.inc"

namespace snout {

__constant__ float kZwXlate[ZW_TAPS_XLATE_N] = {ZW_TAPS_XLATE};
__constant__ float kZwLp[ZW_TAPS_LP_N] = {ZW_TAPS_LP};

static const float kZwMmseHost[129][8] = {
#include "mmse_taps.inc"
};

constexpr int kZwN1 = ZW_TAPS_XLATE_N, kZwN2 = ZW_TAPS_LP_N;
constexpr int kZwTile = 2048;                        // outputs per zw_front workgroup
constexpr int kZwThreads = 256;
constexpr int kZwPer = kZwTile / kZwThreads;         // consecutive outputs of z4 per thread
constexpr int kZwHalo = (kZwN2 - 1) + 1 + (kZwN1 - 1);  // 231 input samples in front of a tile
constexpr int kZwU = kZwTile + kZwHalo;              // mixed input samples of a tile
constexpr int kZwY = kZwTile + kZwN2;                // z2 outputs of a tile (from n0 - 193)
constexpr int kZwD = kZwTile + kZwN2 - 1;            // z3 outputs of a tile (from n0 - 192)
__host__ __device__ constexpr int zw_pad(int j) { return j + (j >> 5); }   // one spare float per 32: 8 consecutive outputs per lane
constexpr int kZwDPad = zw_pad(kZwD) + 1;
constexpr float kZwGain = (float)(2.0 * 800000.0 / (2.0 * 3.14159265358979323846 * 20e3 / 8.0));
static_assert(kZwTile % (kZwThreads * 4) == 0, "tile");
static_assert(kZwDPad <= 2 * kZwU, "d aliases the u buffer");

// z1-z4 fused.  A workgroup turns input samples [n0 - 231, n0 + 2048) into f[n0 .. n0 + 2048): the input is converted and
// mixed into LDS, z1 + z2 write y (LDS), z3 writes d (LDS, over the input buffer), z4 writes f to HBM.  The taps are the
// same for every lane (unrolled constant indices: scalar operands).
template <int FMT>
__global__ __launch_bounds__(kZwThreads) void zw_front(const void* __restrict__ iq, uint32_t n,
                                                       const float* __restrict__ atan_tab, float* __restrict__ f)
{
    __shared__ float2 su[kZwU];          // z1 input; later (as floats) the z3 output
    __shared__ float2 sy[kZwY];
    __shared__ float tab[257];
    const int t = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * kZwTile;
    for (int i = t; i < 257; i += kZwThreads) tab[i] = atan_tab[i];
    for (int i = t; i < kZwU; i += kZwThreads) {
        const int64_t p = n0 - kZwHalo + i;
        float2 x = make_float2(0.0f, 0.0f);
        if (p >= 0 && p < (int64_t)n) x = iq_sample<FMT>(iq, (uint64_t)p);
        const uint32_t r = (uint32_t)p & 3u;            // j^p (p < 0: two's complement keeps p mod 4)
        float2 u;
        if (r == 0u) u = x;
        else if (r == 1u) u = make_float2(-x.y, x.x);
        else if (r == 2u) u = make_float2(-x.x, -x.y);
        else u = make_float2(x.y, -x.x);
        su[i] = u;
    }
    __syncthreads();
    // z1 + z2: y at n0 - 193 + i, its newest input at su[i + 38]
    for (int i = t; i < kZwY; i += kZwThreads) {
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int k = 0; k < kZwN1; k++) {
            const float2 v = su[i + (kZwN1 - 1) - k];
            re = re + kZwXlate[k] * v.x;
            im = im + kZwXlate[k] * v.y;
        }
        const float pw = re * re + im * im;
        const bool open = (double)pw >= 1e-4;
        sy[i] = open ? make_float2(re, im) : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    // z3: d at n0 - 192 + i from y[i + 1] and y[i]
    float* sd = reinterpret_cast<float*>(su);
    for (int i = t; i < kZwD; i += kZwThreads) {
        const float a = zb_discriminate(sy[i + 1], sy[i], tab);
        sd[zw_pad(i)] = kZwGain * a;
    }
    __syncthreads();
    // z4: outputs n0 + kZwPer t + i; d at position n0 + q sits at sd[zw_pad(q + 192)]
    const int q0 = kZwPer * t + (kZwN2 - 1);
    float acc[kZwPer], win[kZwPer];
#pragma unroll
    for (int i = 0; i < kZwPer; i++) { acc[i] = 0.0f; win[i] = sd[zw_pad(q0 + i)]; }
#pragma unroll
    for (int k = 0; k < kZwN2; k++) {
#pragma unroll
        for (int i = 0; i < kZwPer; i++) acc[i] = acc[i] + kZwLp[k] * win[i];
        if (k + 1 < kZwN2) {
#pragma unroll
            for (int i = kZwPer - 1; i > 0; i--) win[i] = win[i - 1];
            win[0] = sd[zw_pad(q0 - k - 1)];
        }
    }
    const int64_t p0 = n0 + kZwPer * t;
    if (p0 + kZwPer <= (int64_t)n) {
        float4* o = reinterpret_cast<float4*>(f + p0);
#pragma unroll
        for (int i = 0; i < kZwPer; i += 4) o[i / 4] = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < kZwPer; i++) if (p0 + i < (int64_t)n) f[p0 + i] = acc[i];
    }
}

// z5-z7, one thread per lane.  Lane k owns the frames whose sample_index (the window start of the symbol that carries the
// SOF's last bit) lies in its core [k C, min((k + 1) C, n)); it starts W samples early with a fresh loop and an empty sink,
// searches while its window starts inside the core, and goes on past the core end only to finish a frame it owns.  A frame
// cut off by the end of the input is dropped.  Records go to the lane's K stage slots (lane_cnt counts past K: overflow).
template <bool TAP>
__global__ __launch_bounds__(64) void zw_lanes(const float* __restrict__ f, uint32_t n, uint32_t core, uint32_t warmup,
                                               uint32_t lane0, uint32_t n_lanes, const float* __restrict__ mmse,
                                               uint32_t channel, uint64_t first, snout_pkt* __restrict__ stage, uint32_t K,
                                               uint32_t* __restrict__ lane_cnt, float* __restrict__ soft,
                                               uint32_t soft_cap, uint32_t* __restrict__ soft_n)
{
    __shared__ float4 tA[129], tB[129];
    for (int i = threadIdx.x; i < 129; i += 64) {
        tA[i] = make_float4(mmse[i * 8 + 0], mmse[i * 8 + 1], mmse[i * 8 + 2], mmse[i * 8 + 3]);
        tB[i] = make_float4(mmse[i * 8 + 4], mmse[i * 8 + 5], mmse[i * 8 + 6], mmse[i * 8 + 7]);
    }
    __syncthreads();
    const uint32_t lane = lane0 + blockIdx.x * 64u + threadIdx.x;
    if (lane >= n_lanes) return;
    const uint64_t cs64 = (uint64_t)lane * core;
    const uint32_t cs = (uint32_t)cs64;                 // < n: the host launches ceil(n / core) lanes
    const uint32_t ce = cs64 + core < n ? (uint32_t)(cs64 + core) : n;
    uint32_t ii = cs > warmup ? cs - warmup : 0u;
    const float omega_mid = 20.0f, gain_omega = (float)(0.25 * 0.175 * 0.175), gain_mu = 0.175f;
    const float omega_lim = omega_mid * 0.005f;
    float mu = 0.5f, omega = 20.0f, last = 0.0f;
    uint32_t reg = 0, cnt = 0, nsym = 0;
    bool reading = false, owned = false;
    uint32_t start = 0, nb = 0, nbits = 0, cur = 0, L = 0, x = 0xFFu, ptype = 0;
    snout_pkt* rec = stage + (size_t)lane * K;
    while (ii + 8u <= n) {
        if (ii >= ce && !(reading && owned)) break;
        const int imu = (int)rintf(mu * 128.0f);
        const float4 ta = tA[imu], tb = tB[imu];
        const float* w = f + ii;
        float acc = 0.0f;
        acc = __builtin_fmaf(ta.x, w[7], acc);
        acc = __builtin_fmaf(ta.y, w[6], acc);
        acc = __builtin_fmaf(ta.z, w[5], acc);
        acc = __builtin_fmaf(ta.w, w[4], acc);
        acc = __builtin_fmaf(tb.x, w[3], acc);
        acc = __builtin_fmaf(tb.y, w[2], acc);
        acc = __builtin_fmaf(tb.z, w[1], acc);
        acc = __builtin_fmaf(tb.w, w[0], acc);
        const float o = acc;
        if constexpr (TAP) { if (nsym < soft_cap) soft[nsym] = o; }
        nsym++;
        const float mm = (last < 0.0f ? -1.0f : 1.0f) * o - (o < 0.0f ? -1.0f : 1.0f) * last;
        last = o;
        omega = omega + gain_omega * mm;
        {
            const float xo = omega - omega_mid;
            const float c = 0.5f * (fabsf(xo + omega_lim) - fabsf(xo - omega_lim));
            omega = omega_mid + c;
        }
        mu = mu + omega + gain_mu * mm;
        const float fl = floorf(mu);
        const uint32_t step = fl >= 1.0f ? (uint32_t)(int)fl : 1u;
        const uint32_t pos = ii;
        ii += step;
        mu = mu - fl;
        // z6 + z7
        const uint32_t bit = o < 0.0f ? 0u : 1u;
        if (!reading) {
            reg = ((reg << 1) | bit) & 0xFFFFFFu;
            if (reg == 0x5555F0u) {
                reading = true;
                start = pos;
                owned = pos >= cs;
                nb = nbits = cur = L = ptype = 0;
                x = 0xFFu;
                if (owned && cnt < K) {
                    uint4* r4 = reinterpret_cast<uint4*>(rec + cnt);
#pragma unroll
                    for (int q = 0; q < 10; q++) r4[q] = make_uint4(0u, 0u, 0u, 0u);
                }
            }
        } else {
            cur = (cur << 1) | bit;
            if (++nbits == 8u) {
                const uint32_t byte = cur;
                cur = nbits = 0;
                if (owned && cnt < K) rec[cnt].bytes[nb] = (uint8_t)byte;
                if (nb == 5u) ptype = byte & 0x0Fu;
                if (nb == 7u) L = byte;
                nb++;
                if (nb == 8u && (L < 10u || L > 64u)) {
                    reading = false;
                    reg = 0;
                } else if (nb >= 8u && nb == L) {
                    if (owned) {
                        if (cnt < K) {
                            snout_pkt* r = rec + cnt;
                            r->sample_index = first + start;
                            r->proto = SNOUT_PROTO_ZWAVE;
                            r->channel = (uint16_t)channel;
                            r->len = (uint16_t)L;
                            r->crc_ok = x == byte ? 1u : 0u;
                            r->lqi = 0;
                            r->pdu_type = (uint8_t)ptype;
                            r->flags = 0;
                            r->aux = lane;
                        }
                        cnt++;
                    }
                    reading = false;
                    reg = 0;
                } else {
                    x ^= byte;
                }
            }
        }
    }
    lane_cnt[lane] = cnt;
    if constexpr (TAP) *soft_n = nsym;
}

// Record offsets: one workgroup, a contiguous run of lanes per thread, exclusive scan of min(count, K).
// totals: [0] lanes, [1] records, [2] 1 if a lane found more than K frames (the host grows K and runs again).
constexpr int kZwScanThreads = 1024;
__global__ __launch_bounds__(kZwScanThreads) void zw_scan(const uint32_t* __restrict__ lane_cnt, uint32_t n_lanes,
                                                          uint32_t K, uint32_t* __restrict__ lane_off,
                                                          uint32_t* __restrict__ totals)
{
    __shared__ uint32_t wsum[kZwScanThreads / 64];
    __shared__ uint32_t wover[kZwScanThreads / 64];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_lanes + kZwScanThreads - 1) / kZwScanThreads;
    const uint32_t a = t * per, b = a + per < n_lanes ? a + per : n_lanes;
    uint32_t s = 0, over = 0;
    for (uint32_t i = a; i < b; i++) {
        const uint32_t c = lane_cnt[i];
        over |= c > K ? 1u : 0u;
        s += c < K ? c : K;
    }
    uint32_t inc = s;
    const uint32_t l = t & 63u, wv = t >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(inc, d);
        if ((int)l >= d) inc += v;
    }
    for (int d = 32; d > 0; d >>= 1) over |= __shfl_xor(over, d);
    if (l == 63u) { wsum[wv] = inc; wover[wv] = over; }
    __syncthreads();
    uint32_t off = inc - s, all = 0, any = 0;
    for (uint32_t w = 0; w < kZwScanThreads / 64; w++) {
        if (w < wv) off += wsum[w];
        all += wsum[w];
        any |= wover[w];
    }
    for (uint32_t i = a; i < b; i++) {
        lane_off[i] = off;
        const uint32_t c = lane_cnt[i];
        off += c < K ? c : K;
    }
    if (t == 0) { totals[0] = n_lanes; totals[1] = all; totals[2] = any; }
}

// One thread per (lane, slot): stage slot -> its place in the ordered output.
__global__ __launch_bounds__(256) void zw_copy(const snout_pkt* __restrict__ stage, const uint32_t* __restrict__ lane_cnt,
                                               const uint32_t* __restrict__ lane_off, uint32_t n_lanes, uint32_t K,
                                               snout_pkt* __restrict__ out, uint32_t out_cap)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = (uint32_t)(g / K), i = (uint32_t)(g % K);
    if (lane >= n_lanes) return;
    const uint32_t c = lane_cnt[lane];
    if (i >= (c < K ? c : K)) return;
    const uint32_t o = lane_off[lane] + i;
    if (o >= out_cap) return;
    const uint4* src = reinterpret_cast<const uint4*>(stage + (size_t)lane * K + i);
    uint4* dst = reinterpret_cast<uint4*>(out + o);
#pragma unroll
    for (int q = 0; q < 10; q++) dst[q] = src[q];
}

// =============================================================================================
// Host side
// =============================================================================================
static inline uint32_t zw_cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

int ZwCtx::init(uint32_t core_, uint32_t warmup_, uint32_t channel_)
{
    core = core_;
    warmup = warmup_;
    channel = channel_;
    std::vector<float> atan_tab(257);
    for (int i = 0; i < 257; i++) atan_tab[i] = (float)atan((double)i / 255.0);
    if (int rc = d_atan.ensure(257 * 4)) return rc;
    if (int rc = d_mmse.ensure(129 * 8 * 4)) return rc;
    SNOUT_HIP(hipMemcpy(d_atan.p, atan_tab.data(), 257 * 4, hipMemcpyHostToDevice));
    SNOUT_HIP(hipMemcpy(d_mmse.p, kZwMmseHost, 129 * 8 * 4, hipMemcpyHostToDevice));
    return 0;
}

void ZwCtx::destroy()
{
    d_atan.release(); d_mmse.release(); d_f.release(); d_stage.release(); d_cnt.release(); d_soft.release();
}

int ZwCtx::enqueue_front(const void* d_iq, uint64_t n, int fmt, hipStream_t st, ResultSlot& s)
{
    if (int rc = d_f.ensure(n * 4u + 64u)) return rc;
    SNOUT_HIP(hipEventRecord(s.ev_k0, st));
    const dim3 grid(zw_cdiv(n, kZwTile));
    if (fmt == kFmtSc8)
        hipLaunchKernelGGL(zw_front<kFmtSc8>, grid, dim3(kZwThreads), 0, st, d_iq, (uint32_t)n, d_atan.as<float>(), d_f.as<float>());
    else if (fmt == kFmtSc16)
        hipLaunchKernelGGL(zw_front<kFmtSc16>, grid, dim3(kZwThreads), 0, st, d_iq, (uint32_t)n, d_atan.as<float>(), d_f.as<float>());
    else
        hipLaunchKernelGGL(zw_front<kFmtCf32>, grid, dim3(kZwThreads), 0, st, d_iq, (uint32_t)n, d_atan.as<float>(), d_f.as<float>());
    SNOUT_HIP(hipGetLastError());
    SNOUT_HIP(hipEventRecord(s.ev_k1, st));
    return 0;
}

int ZwCtx::enqueue_tail(uint64_t n, uint64_t first, hipStream_t st, ResultSlot& s)
{
    n_lanes = zw_cdiv(n, core);
    first_index = first;
    const uint64_t slots = (uint64_t)n_lanes * K;
    if (int rc = s.d_out.ensure(slots * sizeof(snout_pkt))) return rc;
    if (int rc = d_stage.ensure(slots * sizeof(snout_pkt))) return rc;
    if (int rc = d_cnt.ensure((uint64_t)n_lanes * 8u + 64u)) return rc;
    uint32_t* cnt = d_cnt.as<uint32_t>();
    uint32_t* off = cnt + n_lanes;
    hipLaunchKernelGGL(zw_lanes<false>, dim3(zw_cdiv(n_lanes, 64)), dim3(64), 0, st, d_f.as<float>(), (uint32_t)n, core,
                       warmup, 0u, n_lanes, d_mmse.as<float>(), channel, first, d_stage.as<snout_pkt>(), K, cnt,
                       nullptr, 0u, nullptr);
    hipLaunchKernelGGL(zw_scan, dim3(1), dim3(kZwScanThreads), 0, st, cnt, n_lanes, K, off, s.d_totals.as<uint32_t>());
    hipLaunchKernelGGL(zw_copy, dim3(zw_cdiv(slots, 256)), dim3(256), 0, st, d_stage.as<snout_pkt>(), cnt, off, n_lanes, K,
                       s.d_out.as<snout_pkt>(), (uint32_t)(s.d_out.cap / sizeof(snout_pkt)));
    SNOUT_HIP(hipGetLastError());
    return 0;
}

bool ZwCtx::check_overflow(const ResultSlot& s)
{
    if (s.h_totals[2] == 0) return false;
    set_last_error("more than %u Z-Wave frames in one lane", K);
    K *= 4;                   // the caller runs the segment again
    return true;
}

int ZwCtx::soft(uint32_t stage_id, uint32_t lane, uint64_t n, float* out, uint64_t cap, uint64_t* n_out)
{
    *n_out = 0;
    if (stage_id == SNOUT_STAGE_ZW_FILTERED) {
        const uint64_t m = n < cap ? n : cap;
        if (m) SNOUT_HIP(hipMemcpy(out, d_f.p, m * 4u, hipMemcpyDeviceToHost));
        *n_out = n;
        return n > cap ? SNOUT_EOVERFLOW : 0;
    }
    if (stage_id != SNOUT_STAGE_ZW_SYMBOLS || lane >= n_lanes) return SNOUT_EINVAL;
    // the lane again with the tap on (it rewrites its own stage slots and count, identically)
    const uint32_t scap = (uint32_t)(n / 16u + 64u);     // a step is at least 19 samples once the loop runs at omega 20
    if (int rc = d_soft.ensure((uint64_t)scap * 4u + 64u)) return rc;
    uint32_t* sn = reinterpret_cast<uint32_t*>(d_soft.as<float>() + scap);
    hipLaunchKernelGGL(zw_lanes<true>, dim3(1), dim3(64), 0, nullptr, d_f.as<float>(), (uint32_t)n, core, warmup, lane,
                       lane + 1u, d_mmse.as<float>(), channel, first_index, d_stage.as<snout_pkt>(), K, d_cnt.as<uint32_t>(),
                       d_soft.as<float>(), scap, sn);
    SNOUT_HIP(hipGetLastError());
    SNOUT_HIP(hipDeviceSynchronize());
    uint32_t ns = 0;
    SNOUT_HIP(hipMemcpy(&ns, sn, 4, hipMemcpyDeviceToHost));
    const uint64_t have = ns < scap ? ns : scap;
    const uint64_t m = have < cap ? have : cap;
    if (m) SNOUT_HIP(hipMemcpy(out, d_soft.p, m * 4u, hipMemcpyDeviceToHost));
    *n_out = have;
    return have > cap ? SNOUT_EOVERFLOW : 0;
}

}  // namespace snout
