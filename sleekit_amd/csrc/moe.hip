// Mixture-of-experts routing around the grouped products (include/sleekit_amd.h, "MoE routing"): router logits to expert ids
// and gates (slk_moe_topk), the stable counting sort of the ids that the grouped products' offsets come from (slk_moe_sort),
// and the gate-weighted sum back into token order (slk_moe_combine).  The row-mapped activation quantizer, the fourth entry
// of the route, stands beside the plain one in mx.hip.
//
// Two rules hold for every kernel here.  No workgroup waits for another: what one launch needs of another it gets from the
// order of the launches on the caller's stream.  And no address is made from an index read from device memory before that
// index has been checked against its range: a bad index raises the call's flag and neither reads nor writes anything.
#include "common.h"

namespace slk {

typedef unsigned long long u64;

template <class T>
__device__ __forceinline__ float moe_f32(T x);
template <>
__device__ __forceinline__ float moe_f32<float>(float x) { return x; }
template <>
__device__ __forceinline__ float moe_f32<unsigned short>(unsigned short x) { return __uint_as_float((unsigned)x << 16); }
template <>
__device__ __forceinline__ float moe_f32<_Float16>(_Float16 x) { return (float)x; }

static inline bool aligned4(const void *p) { return (uintptr_t)p % 4 == 0; }

constexpr int MOE_MAX_ROWS = 1 << 24;  // n = T k of every entry: int32 indices everywhere, with room to spare

// ---------------------------------------------------------------- top-k
// A float as an unsigned whose order is the float's (-inf lowest of what a row may hold once a NaN has been replaced), and
// back.  Key 0 is below every float: an expert that is not there, or one already taken.
__device__ __forceinline__ unsigned moe_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float moe_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int CTRL>
__device__ __forceinline__ u64 dpp_max64(u64 x) {
    const unsigned lo = (unsigned)dpp_i<CTRL>((int)(unsigned)x), hi = (unsigned)dpp_i<CTRL>((int)(unsigned)(x >> 32));
    const u64 o = ((u64)hi << 32) | lo;
    return o > x ? o : x;
}
__device__ __forceinline__ u64 readlane64(u64 x, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), src);
    return ((u64)hi << 32) | lo;
}
// the wave's largest: four DPP levels make each row of 16 lanes uniform, the four rows meet in scalar registers
__device__ __forceinline__ u64 wave_max64(u64 x) {
    x = dpp_max64<DPP_XOR1>(x);
    x = dpp_max64<DPP_XOR2>(x);
    x = dpp_max64<DPP_HALF_MIRROR>(x);
    x = dpp_max64<DPP_MIRROR>(x);
    const u64 a = readlane64(x, 0), b = readlane64(x, 16), c = readlane64(x, 32), d = readlane64(x, 48);
    const u64 ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}
// the sum of a row of 16 lanes, in every lane of the row: ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) + the same of 8 .. 15
__device__ __forceinline__ float row_sum(float x) {
    x = x + dpp_f<DPP_XOR1>(x);
    x = x + dpp_f<DPP_XOR2>(x);
    x = x + dpp_f<DPP_HALF_MIRROR>(x);
    x = x + dpp_f<DPP_MIRROR>(x);
    return x;
}
__device__ __forceinline__ float readlane_f(float x, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src)); }

// One wave a token, four tokens a workgroup; lane l holds experts l, l + 64, ... (NV of them, 16 at E = 1024) in registers.
// Round j finds the j-th largest: every lane's best (value, lowest index) among what it still holds, then wave_max64 of
// (key of the value) << 32 | ~index, so that of equal values the lower index wins; the winner's lane strikes it out.  -0 is
// read as +0, so the two tie.  A NaN is read as -inf and raises the flag, as +inf does and a k-th value of -inf (fewer than k
// experts left unmasked): the ids are then still k distinct experts of 0 .. E - 1, and the token's gates are 0.
// Gates, float32, every operation rounded once: m the token's largest logit (round 0's), e = expf(v - m),
//   SLK_MOE_GATE_SELECTED: s = the k selected e's, e_j in lane j, summed by row_sum (lanes k .. 15 hold +0);
//   SLK_MOE_GATE_ALL:      s = all E: each lane adds its own in the order l, l + 64, ..., row_sum, then (r0 + r1) + (r2 + r3)
//                          of the four rows: at most 15 + 4 + 2 adds deep;
// g = e / s, the IEEE quotient.  No LDS, no barrier.
template <class T, int NV>
__global__ __launch_bounds__(256) void k_moe_topk(const T *__restrict__ logits, int tokens, int E, int k, int gating,
                                                  int *__restrict__ ids, float *__restrict__ gates, int *__restrict__ flag) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tokens) return;  // (a whole wave: the lanes of the waves that stay are all active)
    const T *row = logits + (size_t)t * E;
    const float ninf = -__builtin_huge_valf();
    float v[NV];
    unsigned key[NV];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i;
        v[i] = ninf, key[i] = 0u;
        if (e < E) {
            float x = moe_f32<T>(row[e]);
            if (x != x) bad = true, x = ninf;
            if (x == __builtin_huge_valf()) bad = true;
            if (x == 0.0f) x = 0.0f;
            v[i] = x, key[i] = moe_key(x);
        }
    }
    int my_id = 0;
    float my_v = ninf, m = ninf, last = ninf;
    for (int j = 0; j < k; ++j) {
        u64 best = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const u64 c = ((u64)key[i] << 32) | (0xffffffffu - (unsigned)(lane + 64 * i));
            best = c > best ? c : best;
        }
        best = wave_max64(best);  // (k <= E: an expert that is there and not taken has a key above 0 and wins)
        const int idx = (int)(0xffffffffu - (unsigned)best);
        last = moe_unkey((unsigned)(best >> 32));
        if (j == 0) m = last;
        if (lane == j) my_id = idx, my_v = last;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (lane + 64 * i == idx) key[i] = 0u;
    }
    bad = __ballot(bad || last == ninf) != 0ull;
    const float e = lane < k ? expf(my_v - m) : 0.0f;
    float s;
    if (gating == SLK_MOE_GATE_SELECTED) {
        s = row_sum(e);
    } else {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float ei = lane + 64 * i < E ? expf(v[i] - m) : 0.0f;
            a = i == 0 ? ei : a + ei;
        }
        a = row_sum(a);
        s = (readlane_f(a, 0) + readlane_f(a, 16)) + (readlane_f(a, 32) + readlane_f(a, 48));
    }
    if (lane < k) {
        ids[(size_t)t * k + lane] = my_id;
        gates[(size_t)t * k + lane] = bad ? 0.0f : e / s;
    }
    if (bad && lane == 0) flag[0] = 1;
}

// ---------------------------------------------------------------- sort
// The stable counting sort of n ids in three launches.  A wave owns a chunk of consecutive entries and walks it 64 at a time.
//   count: every wave's histogram of its chunk (integer atomics in the wave's own LDS counters: sums commute), written
//          expert-major, counts[e C + c] for chunk c of C;
//   scan:  the exclusive prefix sum over that table in its order in memory -- all of expert 0's chunks, then expert 1's --
//          in place, by one workgroup; what stands at (e, 0) is offsets[e];
//   place: every wave loads its column of the table into its LDS counters and walks its chunk again.  A lane's rank among
//          the equal keys of its 64 comes from ceil(log2 E) ballots (the lanes whose key has the same bits), its place is
//          counter + rank, and the last lane of each key adds the key's count to the counter for the next 64.
// Nothing depends on timing: the place of entry i is the number of smaller keys plus the number of equal keys before i.
// n <= MOE_SORT_SMALL takes all three steps in one workgroup of four waves, a chunk of 256 each.
constexpr int MOE_SORT_SMALL = 1024, MOE_SORT_CHUNK = 2048, MOE_SORT_MAX_CHUNKS = 1024;

// entries a wave of the three-launch form: MOE_SORT_CHUNK, or from 2^21 entries up what keeps the chunks at 1024 at the most
// (the table the scan's one workgroup walks is E C ints)
static inline int moe_sort_chunk(int n) {
    const int per = (n + MOE_SORT_MAX_CHUNKS - 1) / MOE_SORT_MAX_CHUNKS;
    return per <= MOE_SORT_CHUNK ? MOE_SORT_CHUNK : (per + 63) / 64 * 64;
}
static inline int moe_sort_chunks(int n) { return (n + moe_sort_chunk(n) - 1) / moe_sort_chunk(n); }
static inline int moe_key_bits(int E) {
    int b = 0;
    while ((1 << b) < E) ++b;
    return b;
}

__device__ __forceinline__ int moe_clamp(int id, int E) { return min(max(id, 0), E - 1); }

// a wave's histogram of entries lo .. hi - 1 into its counters (zeroed by the caller); true where an id is outside 0 .. E - 1
__device__ __forceinline__ bool moe_count_chunk(const int *__restrict__ ids, int lo, int hi, int E, int *cnt) {
    bool bad = false;
    for (int i = lo + (int)(threadIdx.x & 63); i < hi; i += 64) {
        const int id = ids[i];
        bad |= (unsigned)id >= (unsigned)E;
        atomicAdd(&cnt[moe_clamp(id, E)], 1);
    }
    return bad;
}

// a wave places entries lo .. hi - 1 from its counters (the places of its chunk's first entry of every key); true where a
// place is outside 0 .. n - 1, which the counts of the same ids cannot give: nothing is written there
__device__ __forceinline__ bool moe_place_chunk(const int *__restrict__ ids, int lo, int hi, int n, int E, int bits, int *cnt,
                                                int *__restrict__ order, int *__restrict__ pos) {
    const int lane = threadIdx.x & 63;
    const u64 below = (1ull << lane) - 1ull;
    bool bad = false;
    for (int i0 = lo; i0 < hi; i0 += 64) {  // (the same trips for every lane: the ballots take them all)
        const int i = i0 + lane;
        const bool live = i < hi;
        const int key = moe_clamp(live ? ids[i] : 0, E);
        u64 peers = __ballot(live);
        for (int b = 0; b < bits; ++b) {
            const bool set = (key >> b) & 1;
            const u64 with = __ballot(set);
            peers &= set ? with : ~with;
        }
        const int rank = __popcll(peers & below), count = __popcll(peers);
        const int first = live ? cnt[key] : 0;
        __builtin_amdgcn_wave_barrier();  // (every lane has read its counter before the key's last lane moves it on)
        if (live && rank == count - 1) cnt[key] = first + count;
        __builtin_amdgcn_wave_barrier();
        if (live) {
            const unsigned p = (unsigned)(first + rank);
            if (p < (unsigned)n) {
                order[p] = i;
                pos[i] = (int)p;
            } else {
                bad = true;
            }
        }
    }
    return bad;
}

// the exclusive prefix of v over the workgroup's WAVES waves in thread order (sums: WAVES ints of LDS)
template <int WAVES>
__device__ __forceinline__ int block_exclusive_scan(int v, int *sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) sums[wave] = incl;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
        if (w < wave) before += sums[w];
    return before + incl - v;
}

__global__ __launch_bounds__(256) void k_moe_sort_count(const int *__restrict__ ids, int n, int E, int chunk, int chunks,
                                                        int *__restrict__ counts, int *__restrict__ flag) {
    __shared__ int cnt[4 * SLK_MX_MAX_EXPERTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 4 + wave;
    int *mine = cnt + wave * E;
    for (int e = lane; e < E; e += 64) mine[e] = 0;
    __syncthreads();
    bool bad = false;
    if (c < chunks) bad = moe_count_chunk(ids, c * chunk, min(n, (c + 1) * chunk), E, mine);
    __syncthreads();
    if (c < chunks)
        for (int e = lane; e < E; e += 64) counts[(size_t)e * chunks + c] = mine[e];
    if (bad) flag[0] = 1;
}

__global__ __launch_bounds__(1024) void k_moe_sort_scan(int *__restrict__ counts, int E, int chunks, int n, int *__restrict__ offsets) {
    __shared__ int sums[16];
    const int total = E * chunks, per = (total + 1023) / 1024;  // (E C <= 2^20)
    const int lo = min((int)threadIdx.x * per, total), hi = min(lo + per, total);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += counts[i];
    int run = block_exclusive_scan<16>(sum, sums);
    int e = lo / chunks, c = lo - e * chunks;
    for (int i = lo; i < hi; ++i) {
        const int v = counts[i];
        counts[i] = run;
        if (c == 0) offsets[e] = run;
        run += v;
        if (++c == chunks) c = 0, ++e;
    }
    if (threadIdx.x == 0) offsets[E] = n;
}

__global__ __launch_bounds__(256) void k_moe_sort_place(const int *__restrict__ ids, int n, int E, int bits, int chunk, int chunks,
                                                        const int *__restrict__ places, int *__restrict__ order, int *__restrict__ pos,
                                                        int *__restrict__ flag) {
    __shared__ int cnt[4 * SLK_MX_MAX_EXPERTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 4 + wave;
    int *mine = cnt + wave * E;
    if (c < chunks)
        for (int e = lane; e < E; e += 64) mine[e] = places[(size_t)e * chunks + c];
    __syncthreads();
    bool bad = false;
    if (c < chunks) bad = moe_place_chunk(ids, c * chunk, min(n, (c + 1) * chunk), n, E, bits, mine, order, pos);
    if (bad) flag[0] = 1;
}

// the three steps in one workgroup: four waves, wave w the entries 256 w .. 256 w + 255
__global__ __launch_bounds__(256) void k_moe_sort_small(const int *__restrict__ ids, int n, int E, int bits, int *__restrict__ order,
                                                        int *__restrict__ pos, int *__restrict__ offsets, int *__restrict__ flag) {
    __shared__ int cnt[4 * SLK_MX_MAX_EXPERTS];
    __shared__ int sums[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int lo = min(n, wave * (MOE_SORT_SMALL / 4)), hi = min(n, lo + MOE_SORT_SMALL / 4);
    int *mine = cnt + wave * E;
    for (int x = tid; x < 4 * E; x += 256) cnt[x] = 0;
    __syncthreads();
    bool bad = moe_count_chunk(ids, lo, hi, E, mine);
    __syncthreads();
    // thread t scans experts t per .. t per + per - 1, each over the four waves: the table's order, expert-major
    const int per = (E + 255) / 256, e0 = min(E, tid * per), e1 = min(E, e0 + per);
    int sum = 0;
    for (int e = e0; e < e1; ++e)
        for (int w = 0; w < 4; ++w) sum += cnt[w * E + e];
    int run = block_exclusive_scan<4>(sum, sums);
    for (int e = e0; e < e1; ++e) {
        offsets[e] = run;
        for (int w = 0; w < 4; ++w) {
            const int v = cnt[w * E + e];
            cnt[w * E + e] = run;
            run += v;
        }
    }
    if (tid == 0) offsets[E] = n;
    __syncthreads();
    bad |= moe_place_chunk(ids, lo, hi, n, E, bits, mine, order, pos);
    if (bad) flag[0] = 1;
}

// ---------------------------------------------------------------- combine
// out[t][c] = sum_j gates[t][j] * Y[pos[t k + j]][c]: Y to float32, each product rounded, each add rounded, j = 0, 1, ...,
// k - 1, the first term taken as it is (no 0 + ...), the sum rounded once to the output's type.  A thread takes VEC columns
// of one token: a 16-byte piece of Y's row where N is a multiple of the piece (rows then start on 16-byte boundaries, of Y
// and of out alike), otherwise a column.  A pos outside 0 .. T k - 1 raises the flag and its term is left out.
template <class TY, int OUT, int VEC, bool GATED>
__global__ __launch_bounds__(256) void k_moe_combine(const TY *__restrict__ Y, const int *__restrict__ pos, const float *__restrict__ gates,
                                                     size_t units, int k, int N, int n, typename PkOut<OUT>::T *__restrict__ out,
                                                     int *__restrict__ flag) {
    typedef typename PkOut<OUT>::T O;
    typedef TY VI __attribute__((ext_vector_type(VEC)));
    typedef O VO __attribute__((ext_vector_type(VEC), aligned(VEC * sizeof(O) < 16 ? VEC * sizeof(O) : 16)));  // (out is held to 16 bytes, no more)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t per_row = (size_t)N / VEC;
    bool bad = false;
    for (size_t u = gid; u < units; u += threads) {
        const size_t t = u / per_row, c = (u - t * per_row) * VEC;
        float acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
        bool have = false;
        for (int j = 0; j < k; ++j) {
            const int p = pos[t * k + j];
            if ((unsigned)p >= (unsigned)n) {
                bad = true;
                continue;
            }
            float y[VEC];
            if constexpr (VEC == 1) {
                y[0] = moe_f32<TY>(Y[(size_t)p * N + c]);
            } else {
                const VI v = *reinterpret_cast<const VI *>(Y + (size_t)p * N + c);
#pragma unroll
                for (int e = 0; e < VEC; ++e) y[e] = moe_f32<TY>(v[e]);
            }
            if constexpr (GATED) {
                const float g = gates[t * k + j];
#pragma unroll
                for (int e = 0; e < VEC; ++e) y[e] = y[e] * g;
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = have ? acc[e] + y[e] : y[e];
            have = true;
        }
        if constexpr (VEC == 1) {
            out[t * N + c] = PkOut<OUT>::cvt(acc[0]);
        } else {
            VO o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = PkOut<OUT>::cvt(acc[e]);
            *reinterpret_cast<VO *>(out + t * N + c) = o;
        }
    }
    if (bad) flag[0] = 1;
}

static inline int moe_grid(size_t units) {
    size_t b = (units + 255) / 256;
    if (b > 4096) b = 4096;
    return b < 1 ? 1 : (int)b;
}

}  // namespace slk

using namespace slk;

// what the entries of the route refuse of their sizes (functions, because SLK_REQUIRE returns from the one it stands in)
static int moe_check_experts(int E) {
    SLK_REQUIRE(E >= 1 && E <= SLK_MX_MAX_EXPERTS, "E must be 1 .. %d experts (E = %d)", SLK_MX_MAX_EXPERTS, E);
    return SLK_OK;
}
static int moe_check_rows(const char *name, long long rows) {
    SLK_REQUIRE(rows >= 1, "%s must be at least 1 (got %lld)", name, rows);
    SLK_REQUIRE(rows <= MOE_MAX_ROWS, "%s is above the 2^24 routed rows of one call (got %lld)", name, rows);
    return SLK_OK;
}

template <class T>
static int moe_topk_launch(const T *logits, int tokens, int E, int k, int gating, int *ids, float *gates, int *flag, hipStream_t s) {
    const int grid = (tokens + 3) / 4;
    const double bytes = (double)tokens * (E * sizeof(T) + 8.0 * k);
#define SLK_MOE_TOPK(NV) SLK_RUN("moe_topk", 0, bytes, s, (k_moe_topk<T, NV><<<grid, 256, 0, s>>>(logits, tokens, E, k, gating, ids, gates, flag)))
    if (E <= 64) SLK_MOE_TOPK(1);
    else if (E <= 128) SLK_MOE_TOPK(2);
    else if (E <= 256) SLK_MOE_TOPK(4);
    else if (E <= 512) SLK_MOE_TOPK(8);
    else SLK_MOE_TOPK(16);
#undef SLK_MOE_TOPK
    return SLK_OK;
}

extern "C" {

int slk_moe_topk(const void *logits, int dtype, int T, int E, int k, int gating, int *expert_ids, float *gates, int *flag,
                 slk_stream_t stream) {
    SLK_REQUIRE(T >= 1, "T must be at least 1 (got %d)", T);
    if (int rc = moe_check_experts(E)) return rc;
    SLK_REQUIRE(k >= 1 && k <= E && k <= SLK_MOE_MAX_K, "k must be 1 .. min(E, %d) (k = %d, E = %d)", SLK_MOE_MAX_K, k, E);
    if (int rc = moe_check_rows("n = T k", (long long)T * k)) return rc;
    SLK_REQUIRE(known_dtype(dtype), "unknown dtype %d", dtype);
    SLK_REQUIRE(gating == SLK_MOE_GATE_SELECTED || gating == SLK_MOE_GATE_ALL, "unknown gating %d", gating);
    SLK_REQUIRE(logits && expert_ids && gates && flag, "null pointer");
    SLK_REQUIRE((uintptr_t)logits % (dtype == SLK_DTYPE_F32 ? 4 : 2) == 0 && aligned4(expert_ids) && aligned4(gates) && aligned4(flag),
                "logits must be aligned to its element, expert_ids, gates and flag to 4 bytes");
    hipStream_t s = as_stream(stream);
    zero_async(flag, sizeof(int), s);
    return with_dtype(dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T Tl;
        return moe_topk_launch(static_cast<const Tl *>(logits), T, E, k, gating, expert_ids, gates, flag, s);
    });
}

size_t slk_moe_sort_workspace_bytes(int n, int E) {
    if (n < 1 || n > MOE_MAX_ROWS || E < 1 || E > SLK_MX_MAX_EXPERTS || n <= MOE_SORT_SMALL) return 0;
    return sizeof(int) * (size_t)E * moe_sort_chunks(n);
}

int slk_moe_sort(const int *expert_ids, int n, int E, int *order, int *pos, int *offsets, int *flag, void *workspace, size_t ws_bytes,
                 slk_stream_t stream) {
    if (int rc = moe_check_experts(E)) return rc;
    if (int rc = moe_check_rows("n", n)) return rc;
    SLK_REQUIRE(expert_ids && order && pos && offsets && flag, "null pointer");
    SLK_REQUIRE(aligned4(expert_ids) && aligned4(order) && aligned4(pos) && aligned4(offsets) && aligned4(flag),
                "expert_ids, order, pos, offsets and flag must be aligned to 4 bytes");
    const size_t need = slk_moe_sort_workspace_bytes(n, E);
    SLK_REQUIRE(need == 0 || (workspace && aligned4(workspace)), "the workspace must be non-null and aligned to 4 bytes");
    SLK_REQUIRE(ws_bytes >= need, "the workspace is too small: %zu bytes, slk_moe_sort_workspace_bytes(%d, %d) = %zu", ws_bytes, n, E, need);
    hipStream_t s = as_stream(stream);
    zero_async(flag, sizeof(int), s);
    const int bits = moe_key_bits(E);
    const double bytes = 12.0 * n + 4.0 * E;
    if (n <= MOE_SORT_SMALL) {
        SLK_RUN_W("moe_sort_small", 0, bytes, 1, s, k_moe_sort_small<<<1, 256, 0, s>>>(expert_ids, n, E, bits, order, pos, offsets, flag));
        return SLK_OK;
    }
    const int chunk = moe_sort_chunk(n), chunks = moe_sort_chunks(n), grid = (chunks + 3) / 4;
    int *table = static_cast<int *>(workspace);
    const double table_bytes = 4.0 * E * chunks;
    SLK_RUN_W("moe_sort_count", 0, 4.0 * n + table_bytes, grid, s, k_moe_sort_count<<<grid, 256, 0, s>>>(expert_ids, n, E, chunk, chunks, table, flag));
    SLK_RUN_W("moe_sort_scan", 0, 2.0 * table_bytes, 1, s, k_moe_sort_scan<<<1, 1024, 0, s>>>(table, E, chunks, n, offsets));
    SLK_RUN_W("moe_sort_place", 0, bytes + table_bytes, grid, s,
              k_moe_sort_place<<<grid, 256, 0, s>>>(expert_ids, n, E, bits, chunk, chunks, table, order, pos, flag));
    return SLK_OK;
}

int slk_moe_combine(const void *Y, int y_dtype, const int *pos, const float *gates, int T, int k, int N, void *out, int out_dtype, int *flag,
                    slk_stream_t stream) {
    SLK_REQUIRE(T >= 1 && N >= 1, "T and N must be at least 1 (T = %d, N = %d)", T, N);
    SLK_REQUIRE(k >= 1, "k must be at least 1 (got %d)", k);
    if (int rc = moe_check_rows("n = T k", (long long)T * k)) return rc;
    SLK_REQUIRE(known_dtype(y_dtype), "unknown y_dtype %d", y_dtype);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(Y && pos && out && flag, "null pointer");
    SLK_REQUIRE(aligned16(Y) && aligned16(out), "Y and out must be aligned to 16 bytes");
    SLK_REQUIRE(aligned4(pos) && aligned4(gates) && aligned4(flag), "pos, gates and flag must be aligned to 4 bytes");
    hipStream_t s = as_stream(stream);
    zero_async(flag, sizeof(int), s);
    const int n = T * k;
    return with_dtype(y_dtype, [&](auto ti) -> int {
        typedef typename decltype(ti)::T TY;
        return with_dtype(out_dtype, [&](auto to) -> int {
            typedef typename decltype(to)::T O;
            constexpr int OUT = decltype(to)::OUT, PIECE = 16 / (int)sizeof(TY);
            const double bytes = (double)n * N * sizeof(TY) + (double)T * N * sizeof(O) + (gates ? 8.0 : 4.0) * n;
            O *o = static_cast<O *>(out);
            const TY *y = static_cast<const TY *>(Y);
            if (N % PIECE == 0) {
                const size_t units = (size_t)T * (N / PIECE);
                if (gates)
                    SLK_RUN("moe_combine", 0, bytes, s, (k_moe_combine<TY, OUT, PIECE, true><<<moe_grid(units), 256, 0, s>>>(y, pos, gates, units, k, N, n, o, flag)));
                else
                    SLK_RUN("moe_combine", 0, bytes, s, (k_moe_combine<TY, OUT, PIECE, false><<<moe_grid(units), 256, 0, s>>>(y, pos, gates, units, k, N, n, o, flag)));
            } else {
                const size_t units = (size_t)T * N;
                if (gates)
                    SLK_RUN("moe_combine", 0, bytes, s, (k_moe_combine<TY, OUT, 1, true><<<moe_grid(units), 256, 0, s>>>(y, pos, gates, units, k, N, n, o, flag)));
                else
                    SLK_RUN("moe_combine", 0, bytes, s, (k_moe_combine<TY, OUT, 1, false><<<moe_grid(units), 256, 0, s>>>(y, pos, gates, units, k, N, n, o, flag)));
            }
            return SLK_OK;
        });
    });
}

}  // extern "C"
