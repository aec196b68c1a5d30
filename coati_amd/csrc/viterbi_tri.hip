// viterbi_tri: pairwise alignment under the triplet models (tri-mg, tri-ecm, dna).
//
// What it replaces in the reference:
//   fst_alignment / evo_fst       src/lib/align_fst.cc:46-160  (compose, ShortestPath, ShortestDistance, TopSort)
//   mg94 / dna / indel / add_arc  src/lib/mutation_fst.cc;  ecm  src/lib/mutation_ecm.cc:194-218
//
// The reference builds ancestor FSA o (mutation FST o indel FST) o descendant FSA and takes its shortest path.
// In the tropical semiring that is the minimum, over every choice of mutated sense codon c' per ancestor codon
// c and every path of indel()'s machine over the mutated nucleotides x', of the summed arc weights.  This file
// computes that minimum as a DP:
//   S(i,j)    at indel() state `start` after i mutated nucleotides and j descendant characters (a match, or (0,0))
//   I(i,j)    inside an insertion run, y_j just inserted
//   D(i,j)    inside a deletion run, x'_i just deleted
//   Mid = min(S + no_gap, I + close)          (no insertion / end of the insertion run)
//   M0  = min(Mid + no_gap, D + close)        (no deletion / end of the deletion run: ready to match or end)
//   Dp  = min(Mid + open, D + ext)            (the deletion run goes on with the next x')
//   I(i,j) = min(S(i,j-1) + open, I(i,j-1) + ext) + pi(y_j)
//   S(i,j) = M0(i-1,j-1) + match(x'_i, y_j)   D(i,j) = Dp(i-1,j)
//   score  = M0(n, m)                         (`end` is free)
// Codon models: every value carries the prefix of c' written so far in the current codon (1, 4 or 16 values for
// i mod 3 = 0, 1, 2); completing the codon adds cost(c, c') and keeps the minimum over the 61 sense c'.
// dna: x' is chosen per nucleotide at cost(x, x'); no prefix.
//
// Machine: one wavefront per pair, four per 256-thread block (the 64x64 cost table in LDS is shared by them).
// Lane L of pass P owns ancestor codon k = 64P + L -- its three rows of cells -- and sweeps the descendant
// columns with one step of skew per lane; the values of the codon's last row (Mid, D) go to lane L+1 by a
// shuffle each step, lane 63's go to the next pass through a per-pass HBM boundary row.  All lanes run the
// same code (no per-phase divergence).  Every cell's decisions are stored (16 B per codon row and column,
// coalesced: a step's 64 records are contiguous); lane 0 then walks them back.  Ties: the first candidate
// wins -- S before I for Mid, Mid before D for M0 and Dp, open before extend for I, the lowest c' (AAA..TTT
// order) for a codon -- so a pair's alignment does not depend on its batch.
#include "abi_internal.hpp"

#include <cmath>
#include <climits>
#include <cstring>

struct coati_hip_triplet_model {
    int device = 0;
    int kind = 0;
    float k[10] = {};  // TriConsts, see below
    float* d_table = nullptr;
    hipStream_t stream = nullptr;
};

namespace {

constexpr float kInf = __builtin_inff();

struct TriConsts {
    float no_gap, open, ext, close;  // -log(1-g), -log g, -log e, -log(1-e)
    float match, mismatch;           // -log(1-3b), -log b
    float pi[4];                     // -log pi (inserted A C G T; N costs 0)
};
static_assert(sizeof(TriConsts) == 10 * sizeof(float), "TriConsts layout");

struct TriArgs {
    const uint8_t* a;
    const uint64_t* a_off;
    const uint8_t* b;
    const uint64_t* b_off;
    const float* table;      // codon: 64x64 (c64, c'64), +inf in stop rows/columns; dna: 4x4
    uint8_t* dec;            // decision records
    const uint64_t* dec_off; // per pair, bytes
    float* bnd;              // pass boundary rows
    const uint64_t* bnd_off; // per pair, floats
    float* scores;
    uint8_t* ops;            // per pair a slot of len_a + len_b bytes, filled from its end
    const uint64_t* ops_off; // slot starts
    uint32_t* ops_len;
    uint32_t n_pairs;
    TriConsts k;
};

// records: codon models 16 B (word 0: row 1 nibbles z=0..3 in bits 0-15, row 3 nibble in 16-19, c'_S in 20-25,
// c'_D in 26-31; words 1-2: row 2 nibbles q=0..15); dna 4 B (nibbles of rows 1, 2, 3 in bits 0-11).
// Nibble: bit 0 Mid took I, bit 1 M0 took D, bit 2 Dp took D, bit 3 I extended.
template <bool CODON> struct RecOf;
template <> struct RecOf<true> { using T = uint4; };
template <> struct RecOf<false> { using T = uint32_t; };

__host__ __device__ inline uint64_t bnd_stride(uint64_t m) { return (2 * (m + 1) + 31) & ~uint64_t{31}; }  // floats, 128 B rows
__host__ __device__ inline uint64_t n_passes(uint64_t n) { return n < 3 ? 1 : (n / 3 + 63) / 64; }

// one cell's indel-state update; returns its nibble
__device__ __forceinline__ uint32_t cell(float S, float D, float& Sprev, float& Iprev, float piy, const TriConsts& k,
                                         float& mid, float& m0, float& dp) {
    const float io = Sprev + k.open, ie = Iprev + k.ext;
    const uint32_t d = ie < io;
    const float I = (d ? ie : io) + piy;
    const float ms = S + k.no_gap, mi = I + k.close;
    const uint32_t a = mi < ms;
    mid = a ? mi : ms;
    const float bm = mid + k.no_gap, bd = D + k.close;
    const uint32_t b = bd < bm;
    m0 = b ? bd : bm;
    const float cm = mid + k.open, cd = D + k.ext;
    const uint32_t c = cd < cm;
    dp = c ? cd : cm;
    Sprev = S;
    Iprev = I;
    return a | (b << 1) | (c << 2) | (d << 3);
}

template <bool CODON>
__global__ __launch_bounds__(256) void viterbi_tri_kernel(TriArgs g) {
    using Rec = typename RecOf<CODON>::T;
    constexpr int kTab = CODON ? 64 * 64 : 16;
    __shared__ float tab[kTab];
    for(int t = threadIdx.x; t < kTab; t += blockDim.x) tab[t] = g.table[t];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    if(pair >= g.n_pairs) return;  // (whole wavefronts; no barrier below)
    const TriConsts k = g.k;
    const uint8_t* A = g.a + g.a_off[pair];
    const uint8_t* B = g.b + g.b_off[pair];
    const int n = static_cast<int>(g.a_off[pair + 1] - g.a_off[pair]);
    const int m = static_cast<int>(g.b_off[pair + 1] - g.b_off[pair]);
    const int K = n / 3;
    const int passes = static_cast<int>(n_passes(n));
    Rec* dec = reinterpret_cast<Rec*>(g.dec + g.dec_off[pair]);
    float* bnd = g.bnd + g.bnd_off[pair];
    const uint64_t stride = bnd_stride(m);

    for(int P = 0; P < passes; ++P) {
        const int kr = P * 64 + lane;
        const bool row_live = kr < K;
        int x0 = 0, x1 = 0, x2 = 0;
        if(row_live) x0 = A[3 * kr], x1 = A[3 * kr + 1], x2 = A[3 * kr + 2];
        const int c64 = x0 * 16 + x1 * 4 + x2;
        // previous column, per row of the codon
        float S1p[CODON ? 4 : 1], I1p[CODON ? 4 : 1], M01p[CODON ? 4 : 1];
        float S2p[CODON ? 16 : 1], I2p[CODON ? 16 : 1], M02p[CODON ? 16 : 1];
        float S3p = kInf, I3p = kInf, M0Ap = kInf;
#pragma unroll
        for(int z = 0; z < (CODON ? 4 : 1); ++z) S1p[z] = I1p[z] = M01p[z] = kInf;
#pragma unroll
        for(int q = 0; q < (CODON ? 16 : 1); ++q) S2p[q] = I2p[q] = M02p[q] = kInf;
        float S0p = kInf, I0p = kInf;  // row 0 (lane 0 of pass 0)
        float upMid = kInf, upD = kInf;
        const float* bin = bnd + static_cast<uint64_t>(P > 0 ? P - 1 : 0) * stride;
        float* bout = bnd + static_cast<uint64_t>(P) * stride;
        for(int s = 0; s <= m + 63; ++s) {
            const int j = s - lane;
            const bool col_live = j >= 0 && j <= m;
            const int y = (j >= 1 && col_live) ? B[j - 1] : 4;
            const float piy = y == 0 ? k.pi[0] : y == 1 ? k.pi[1] : y == 2 ? k.pi[2] : y == 3 ? k.pi[3] : 0.0f;  // (no dynamic index: keeps k in registers)
            float MidA = upMid, DA = upD;
            if(lane == 0 && col_live) {
                if(P == 0) {
                    float m0r, dpr;
                    (void)cell(j == 0 ? 0.0f : kInf, kInf, S0p, I0p, piy, k, MidA, m0r, dpr);
                    DA = kInf;
                    if(K == 0 && j == m) g.scores[pair] = m0r;
                } else {
                    MidA = __hip_atomic_load(bin + 2 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    DA = __hip_atomic_load(bin + 2 * j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            float outMid = kInf, outD = kInf;
            if(col_live && row_live) {
                float mc[4];
#pragma unroll
                for(int z = 0; z < 4; ++z) mc[z] = y == 4 ? 0.0f : (z == y ? k.match : k.mismatch);
                const float bm = MidA + k.no_gap, bd = DA + k.close;
                const float M0A = bd < bm ? bd : bm;
                const float cm = MidA + k.open, cd = DA + k.ext;
                const float DpA = cd < cm ? cd : cm;
                Rec rec;
                if constexpr(CODON) {
                    // row 1: prefix z
                    uint32_t w0 = 0, w1 = 0, w2 = 0;
                    float M01[4], Dp1[4];
#pragma unroll
                    for(int z = 0; z < 4; ++z) {
                        float mid;
                        w0 |= cell(M0Ap + mc[z], DpA, S1p[z], I1p[z], piy, k, mid, M01[z], Dp1[z]) << (4 * z);
                    }
                    // row 2: prefix q = 4p + z
                    float M02[16], Dp2[16];
#pragma unroll
                    for(int q = 0; q < 16; ++q) {
                        float mid;
                        const uint32_t nib = cell(M01p[q >> 2] + mc[q & 3], Dp1[q >> 2], S2p[q], I2p[q], piy, k, mid, M02[q], Dp2[q]);
                        if(q < 8) w1 |= nib << (4 * q);
                        else w2 |= nib << (4 * (q - 8));
                    }
                    // row 3: the codon completes; minimum over the sense codons c'
                    const float* row = tab + c64 * 64;
                    float S3 = kInf, D3 = kInf;
                    uint32_t cs = 0, cdd = 0;
#pragma unroll
                    for(int c = 0; c < 64; c += 4) {
                        const float4 t = *reinterpret_cast<const float4*>(row + c);
                        const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                        for(int z = 0; z < 4; ++z) {
                            const float vs = (M02p[c >> 2] + mc[z]) + tv[z];
                            const float vd = Dp2[c >> 2] + tv[z];
                            if(vs < S3) S3 = vs, cs = c + z;
                            if(vd < D3) D3 = vd, cdd = c + z;
                        }
                    }
                    float M03, Dp3;
                    w0 |= cell(S3, D3, S3p, I3p, piy, k, outMid, M03, Dp3) << 16;
                    w0 |= cs << 20 | cdd << 26;
                    outD = D3;
#pragma unroll
                    for(int z = 0; z < 4; ++z) M01p[z] = M01[z];
#pragma unroll
                    for(int q = 0; q < 16; ++q) M02p[q] = M02[q];
                    rec = make_uint4(w0, w1, w2, 0u);
                    if(kr == K - 1 && j == m) g.scores[pair] = M03;
                } else {
                    // dna: x' per nucleotide at cost tab[x][x']
                    uint32_t w = 0;
                    float M0r[3], Dpr[3], Dr[3], mid = kInf;
                    // row r from: M0 of row r-1 at column j-1, Dp of row r-1 at column j
                    auto row = [&](int x, float M0in, float Dpin, float& Sp, float& Ip, int r) {
                        const float* t = tab + 4 * x;
                        float S = kInf, Dm = kInf;
#pragma unroll
                        for(int z = 0; z < 4; ++z) {
                            const float vs = (M0in + mc[z]) + t[z];
                            const float vd = Dpin + t[z];
                            if(vs < S) S = vs;
                            if(vd < Dm) Dm = vd;
                        }
                        w |= cell(S, Dm, Sp, Ip, piy, k, mid, M0r[r], Dpr[r]) << (4 * r);
                        Dr[r] = Dm;
                    };
                    row(x0, M0Ap, DpA, S1p[0], I1p[0], 0);
                    row(x1, M01p[0], Dpr[0], S2p[0], I2p[0], 1);
                    row(x2, M02p[0], Dpr[1], S3p, I3p, 2);
                    M01p[0] = M0r[0];
                    M02p[0] = M0r[1];
                    outMid = mid;
                    outD = Dr[2];
                    rec = w;
                    if(kr == K - 1 && j == m) g.scores[pair] = M0r[2];
                }
                dec[(static_cast<uint64_t>(P) * (m + 64) + s) * 64 + lane] = rec;
                M0Ap = M0A;
                if(lane == 63 && P + 1 < passes) {
                    __hip_atomic_store(bout + 2 * j, outMid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(bout + 2 * j + 1, outD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            upMid = __shfl_up(outMid, 1, 64);
            upD = __shfl_up(outD, 1, 64);
        }
        __threadfence();
    }
    if(lane != 0) return;

    // traceback from M0(n, m)
    enum { ST_M0, ST_MID, ST_DP, ST_S, ST_I, ST_D };
    uint8_t* ops = g.ops + g.ops_off[pair];
    int w = n + m, i = n, j = m, st = ST_M0, p = 0;
    bool ok = true;
    for(int guard = 0; guard < 4 * (n + m) + 8; ++guard) {
        uint32_t nib = 0, cs = 0, cdd = 0;
        const int r = (i - 1) % 3;
        if(i > 0) {
            const int kr = (i - 1) / 3, P = kr / 64, L = kr % 64;
            const uint64_t at = (static_cast<uint64_t>(P) * (m + 64) + j + L) * 64 + L;
            if constexpr(CODON) {
                const uint4 rec = reinterpret_cast<const uint4*>(dec)[at];
                if(r == 0) nib = rec.x >> (4 * p);
                else if(r == 1) nib = p < 8 ? rec.y >> (4 * p) : rec.z >> (4 * (p - 8));
                else nib = rec.x >> 16, cs = (rec.x >> 20) & 63, cdd = rec.x >> 26;
            } else {
                nib = reinterpret_cast<const uint32_t*>(dec)[at] >> (4 * r);
            }
        } else {
            // row 0: S(0,0) = 0, then insertions only (D and every S but (0,0) are +inf there)
            nib = 0x1u | (j > 1 ? 0x8u : 0u);
            if(j == 0) nib = 0;
        }
        if(st == ST_M0) {
            st = (nib & 2) ? ST_D : ST_MID;
        } else if(st == ST_MID) {
            st = (nib & 1) ? ST_I : ST_S;
        } else if(st == ST_DP) {
            st = (nib & 4) ? ST_D : ST_MID;
        } else if(st == ST_I) {
            if(j < 1 || w < 1) { ok = false; break; }
            ops[--w] = COATI_HIP_OP_INS;
            --j;
            st = (nib & 8) ? ST_I : ST_S;
        } else {  // ST_S or ST_D
            if(st == ST_S && i == 0 && j == 0) break;
            if(i < 1 || w < 1 || (st == ST_S && j < 1)) { ok = false; break; }
            const bool del = st == ST_D;
            ops[--w] = del ? COATI_HIP_OP_DEL : COATI_HIP_OP_MATCH;
            if(CODON) p = r == 0 ? 0 : (r == 1 ? p >> 2 : static_cast<int>((del ? cdd : cs) >> 2));
            --i;
            if(!del) --j;
            st = del ? ST_DP : ST_M0;
        }
    }
    if(!(i == 0 && j == 0 && st == ST_S)) ok = false;
    g.ops_len[pair] = static_cast<uint32_t>(n + m - w);
    if(!ok) g.scores[pair] = __builtin_nanf("");
}

// add_arc's weight of a probability (mutation_fst.cc: 1 -> 0, 0 -> INT_MAX, else -logf)
float arc_weight(float p) {
    if(p == 1.0f) return 0.0f;
    if(p == 0.0f) return static_cast<float>(INT_MAX);
    return -::logf(p);
}

bool triplet_device_ok(int dev) {
    hipDeviceProp_t prop;
    if(hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

uint64_t dec_bytes(bool codon, uint64_t n, uint64_t m) { return n_passes(n) * (m + 64) * 64 * (codon ? 16 : 4); }

}  // namespace

using coati_hip_abi::fail;

extern "C" {

int coati_hip_triplet_model_create(int kind, const float* cost_table, float gap_open, float gap_extend, const float pi[4],
                                   float bc_error, int device, coati_hip_triplet_model_t** out) {
    if(out == nullptr) return fail(COATI_HIP_EINVAL, "triplet_model_create: out is NULL");
    *out = nullptr;
    if(kind != COATI_HIP_TRIPLET_CODON && kind != COATI_HIP_TRIPLET_DNA)
        return fail(COATI_HIP_EINVAL, "triplet_model_create: unknown kind %d", kind);
    if(cost_table == nullptr || pi == nullptr) return fail(COATI_HIP_EINVAL, "triplet_model_create: NULL table or pi");
    const bool codon = kind == COATI_HIP_TRIPLET_CODON;
    const int side = codon ? 61 : 4;
    for(int t = 0; t < side * side; ++t)
        if(std::isnan(cost_table[t]) || std::isinf(cost_table[t]))
            return fail(COATI_HIP_EINVAL, "triplet_model_create: cost_table[%d] is not finite", t);
    if(!(gap_open > 0.0f && gap_open < 1.0f) || !(gap_extend > 0.0f && gap_extend < 1.0f))
        return fail(COATI_HIP_EINVAL, "triplet_model_create: gap probabilities must be in (0,1)");
    if(!(bc_error > 0.0f && 1 - 3 * bc_error >= 0.0f))
        return fail(COATI_HIP_EINVAL, "triplet_model_create: bc_error must be in (0,1/3]");
    for(int q = 0; q < 4; ++q)
        if(!(pi[q] >= 0.0f && pi[q] <= 1.0f)) return fail(COATI_HIP_EINVAL, "triplet_model_create: pi[%d] not in [0,1]", q);
    TriConsts k;
    // indel() (mutation_fst.cc): the same float expressions the reference hands to add_arc
    k.no_gap = arc_weight(1.0f - gap_open);
    k.open = arc_weight(gap_open);
    k.ext = arc_weight(gap_extend);
    k.close = arc_weight(1.0f - gap_extend);
    k.match = arc_weight(1 - 3 * bc_error);
    k.mismatch = arc_weight(bc_error);
    for(int q = 0; q < 4; ++q) k.pi[q] = arc_weight(pi[q]);
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(COATI_HIP_ENODEVICE, "triplet_model_create: no HIP device available");
    if(device < 0 || device >= n) return fail(COATI_HIP_EINVAL, "triplet_model_create: device %d out of range [0,%d)", device, n);
    if(!triplet_device_ok(device)) return fail(COATI_HIP_ENODEVICE, "triplet_model_create: device %d is not gfx950 (MI355X)", device);
    // the device table: codon models 64x64 over the 64-codon index (stop rows / columns +inf), dna 4x4
    std::vector<float> tab(codon ? 64 * 64 : 16, kInf);
    if(codon) {
        int c61 = 0;
        int map[64];
        for(int c = 0; c < 64; ++c) map[c] = (c == 48 || c == 50 || c == 56) ? -1 : c61++;
        for(int c = 0; c < 64; ++c)
            for(int d = 0; d < 64; ++d)
                if(map[c] >= 0 && map[d] >= 0) tab[c * 64 + d] = cost_table[map[c] * 61 + map[d]];
    } else {
        std::memcpy(tab.data(), cost_table, 16 * sizeof(float));
    }
    auto* mdl = new(std::nothrow) coati_hip_triplet_model;
    if(mdl == nullptr) return fail(COATI_HIP_ENOMEM, "triplet_model_create: host allocation failed");
    mdl->device = device;
    mdl->kind = kind;
    std::memcpy(mdl->k, &k, sizeof k);
    auto cleanup = [&](int rc) {
        coati_hip_triplet_model_destroy(mdl);
        return rc;
    };
    hipError_t e;
    if((e = hipSetDevice(device)) != hipSuccess) return cleanup(fail(COATI_HIP_EHIP, "hipSetDevice: %s", hipGetErrorString(e)));
    if((e = hipStreamCreateWithFlags(&mdl->stream, hipStreamNonBlocking)) != hipSuccess)
        return cleanup(fail(COATI_HIP_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    if((e = hipMalloc(&mdl->d_table, tab.size() * sizeof(float))) != hipSuccess)
        return cleanup(fail(COATI_HIP_ENOMEM, "hipMalloc(table): %s", hipGetErrorString(e)));
    if((e = hipMemcpy(mdl->d_table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
        return cleanup(fail(COATI_HIP_EHIP, "hipMemcpy(table): %s", hipGetErrorString(e)));
    *out = mdl;
    return COATI_HIP_OK;
}

void coati_hip_triplet_model_destroy(coati_hip_triplet_model_t* model) {
    if(model == nullptr) return;
    (void)hipSetDevice(model->device);
    if(model->d_table != nullptr) (void)hipFree(model->d_table);
    if(model->stream != nullptr) (void)hipStreamDestroy(model->stream);
    delete model;
}

int coati_hip_triplet_align(coati_hip_triplet_model_t* model, uint64_t n_pairs, const uint8_t* a_cat, const uint64_t* a_off,
                            const uint8_t* b_cat, const uint64_t* b_off, float* scores, uint8_t* ops, uint64_t ops_cap,
                            uint64_t* ops_off, uint32_t* ops_len) {
    if(model == nullptr) return fail(COATI_HIP_EINVAL, "triplet_align: model is NULL");
    if(n_pairs == 0) return COATI_HIP_OK;
    if(a_off == nullptr || b_off == nullptr || scores == nullptr || ops == nullptr || ops_off == nullptr || ops_len == nullptr)
        return fail(COATI_HIP_EINVAL, "triplet_align: NULL argument");
    const bool codon = model->kind == COATI_HIP_TRIPLET_CODON;
    uint64_t slots = 0;
    for(uint64_t p = 0; p < n_pairs; ++p) {
        if(a_off[p + 1] < a_off[p] || b_off[p + 1] < b_off[p]) return fail(COATI_HIP_EINVAL, "triplet_align: offsets of pair %llu decrease", (unsigned long long)p);
        const uint64_t la = a_off[p + 1] - a_off[p], lb = b_off[p + 1] - b_off[p];
        if(la % 3 != 0) return fail(COATI_HIP_EINVAL, "triplet_align: ancestor of pair %llu is not a whole number of codons", (unsigned long long)p);
        if(la > (1u << 30) || lb > (1u << 30)) return fail(COATI_HIP_EINVAL, "triplet_align: pair %llu too long", (unsigned long long)p);
        for(uint64_t t = a_off[p]; t < a_off[p + 1]; ++t)
            if(a_cat[t] > 3) return fail(COATI_HIP_EINVAL, "triplet_align: ancestor code %u of pair %llu out of range", a_cat[t], (unsigned long long)p);
        for(uint64_t t = a_off[p]; t < a_off[p + 1]; t += 3) {
            const int c = a_cat[t] * 16 + a_cat[t + 1] * 4 + a_cat[t + 2];
            if(c == 48 || c == 50 || c == 56) return fail(COATI_HIP_EINVAL, "triplet_align: stop codon in the ancestor of pair %llu", (unsigned long long)p);
        }
        for(uint64_t t = b_off[p]; t < b_off[p + 1]; ++t)
            if(b_cat[t] > 4) return fail(COATI_HIP_EINVAL, "triplet_align: descendant code %u of pair %llu out of range", b_cat[t], (unsigned long long)p);
        slots += la + lb;
    }
    if(ops_cap < slots) return fail(COATI_HIP_EINVAL, "triplet_align: ops_cap %llu < %llu", (unsigned long long)ops_cap, (unsigned long long)slots);
    HIP_TRY(hipSetDevice(model->device));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // decisions of one launch: at most 16 GB and half of what is free; a larger pair goes alone
    const uint64_t budget = std::min<uint64_t>(16ull << 30, free_b / 2);
    uint64_t slot = 0;
    for(uint64_t p0 = 0; p0 < n_pairs;) {
        // plan the chunk [p0, p1)
        uint64_t p1 = p0, need = 0;
        std::vector<uint64_t> h_dec_off, h_bnd_off, h_ops_off, h_a_off, h_b_off;
        uint64_t dec_tot = 0, bnd_tot = 0, ops_tot = 0;
        while(p1 < n_pairs) {
            const uint64_t la = a_off[p1 + 1] - a_off[p1], lb = b_off[p1 + 1] - b_off[p1];
            const uint64_t d = dec_bytes(codon, la, lb), bb = n_passes(la) * bnd_stride(lb) * 4;
            const uint64_t add = d + bb + la + lb + la + lb + 64;
            if(p1 > p0 && need + add > budget) break;
            need += add;
            ++p1;
        }
        const uint64_t cnt = p1 - p0;
        for(uint64_t p = p0; p < p1; ++p) {
            const uint64_t la = a_off[p + 1] - a_off[p], lb = b_off[p + 1] - b_off[p];
            h_dec_off.push_back(dec_tot);
            h_bnd_off.push_back(bnd_tot);
            h_ops_off.push_back(ops_tot);
            h_a_off.push_back(a_off[p] - a_off[p0]);
            h_b_off.push_back(b_off[p] - b_off[p0]);
            dec_tot += (dec_bytes(codon, la, lb) + 255) & ~uint64_t{255};
            bnd_tot += n_passes(la) * bnd_stride(lb);
            ops_tot += la + lb;
        }
        h_a_off.push_back(a_off[p1] - a_off[p0]);
        h_b_off.push_back(b_off[p1] - b_off[p0]);
        const uint64_t na = h_a_off.back(), nb = h_b_off.back();
        // one device block: [dec | bnd | offsets (6 arrays) | scores | ops_len | ops | a | b]
        auto up = [](uint64_t x) { return (x + 255) & ~uint64_t{255}; };
        const uint64_t o_bnd = up(dec_tot), o_offs = o_bnd + up(bnd_tot * 4), o_sc = o_offs + up((5 * cnt + 2) * 8);
        const uint64_t o_len = o_sc + up(cnt * 4), o_ops = o_len + up(cnt * 4), o_a = o_ops + up(ops_tot + 1), o_b = o_a + up(na + 1);
        const uint64_t bytes = o_b + up(nb + 1);
        uint8_t* blk = nullptr;
        HIP_TRY(hipMalloc(&blk, bytes));
        std::vector<uint64_t> offs;
        offs.insert(offs.end(), h_a_off.begin(), h_a_off.end());
        offs.insert(offs.end(), h_b_off.begin(), h_b_off.end());
        offs.insert(offs.end(), h_dec_off.begin(), h_dec_off.end());
        offs.insert(offs.end(), h_bnd_off.begin(), h_bnd_off.end());
        offs.insert(offs.end(), h_ops_off.begin(), h_ops_off.end());
        hipStream_t st = model->stream;
        auto run = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(blk + o_offs, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, st));
            if(na > 0) HIP_TRY(hipMemcpyAsync(blk + o_a, a_cat + a_off[p0], na, hipMemcpyHostToDevice, st));
            if(nb > 0) HIP_TRY(hipMemcpyAsync(blk + o_b, b_cat + b_off[p0], nb, hipMemcpyHostToDevice, st));
            const uint64_t* d_offs = reinterpret_cast<const uint64_t*>(blk + o_offs);
            TriArgs g;
            g.a = blk + o_a;
            g.a_off = d_offs;
            g.b = blk + o_b;
            g.b_off = d_offs + (cnt + 1);
            g.table = model->d_table;
            g.dec = blk;
            g.dec_off = d_offs + 2 * (cnt + 1);
            g.bnd = reinterpret_cast<float*>(blk + o_bnd);
            g.bnd_off = d_offs + 2 * (cnt + 1) + cnt;
            g.scores = reinterpret_cast<float*>(blk + o_sc);
            g.ops = blk + o_ops;
            g.ops_off = d_offs + 2 * (cnt + 1) + 2 * cnt;
            g.ops_len = reinterpret_cast<uint32_t*>(blk + o_len);
            g.n_pairs = static_cast<uint32_t>(cnt);
            std::memcpy(&g.k, model->k, sizeof g.k);
            const dim3 grid(static_cast<uint32_t>((cnt + 3) / 4)), block(256);
            if(codon)
                hipLaunchKernelGGL(viterbi_tri_kernel<true>, grid, block, 0, st, g);
            else
                hipLaunchKernelGGL(viterbi_tri_kernel<false>, grid, block, 0, st, g);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(scores + p0, g.scores, cnt * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(ops_len + p0, g.ops_len, cnt * 4, hipMemcpyDeviceToHost, st));
            if(ops_tot > 0) HIP_TRY(hipMemcpyAsync(ops + slot, g.ops, ops_tot, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return COATI_HIP_OK;
        };
        const int rc = run();
        (void)hipFree(blk);
        if(rc != COATI_HIP_OK) return rc;
        for(uint64_t q = 0; q < cnt; ++q) {
            const uint64_t p = p0 + q, la = a_off[p + 1] - a_off[p], lb = b_off[p + 1] - b_off[p];
            if(std::isnan(scores[p]) || ops_len[p] > la + lb)
                return fail(COATI_HIP_EHIP, "triplet_align: the traceback of pair %llu did not reach (0,0)", (unsigned long long)p);
            ops_off[p] = slot + h_ops_off[q] + (la + lb - ops_len[p]);
        }
        slot += ops_tot;
        p0 = p1;
    }
    return COATI_HIP_OK;
}

}  // extern "C"
