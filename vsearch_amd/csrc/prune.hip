// prune.hip -- index pruning: a NEW index holding, for every row of a CSR index, a pinned subset of its stored cells (vs_index_prune; the
// semantics are pinned in vsearch_hip.h).  The reference fixes a document's sparsity when it embeds it -- embed(..., topk = 768), mask =
// bow_mask | topk_mask (encoder/vdr.py:102-168) --; the stored rows hold everything a smaller topk needs, so the index built with topk = m is
// made here from the index built with topk = 768 and the bag-of-token rows (the protect index).  Three steps on the source's GPU: select (a
// keep byte a source packet, a kept count a row), scan (row pointers from the kept counts: the shared pair of new_index.h), pack.  The
// scaffold of the call is new_index.h.  Nothing here touches a walk or scan kernel.
#include "common.h"
#include "new_index.h"
#include "prune_check.h"

#include <algorithm>
#include <cmath>

using namespace vs;

namespace {

// this wave's LDS writes precede its LDS reads behind this point (LDS executes a wave's operations in order; the fence keeps the compiler's
// order and waits for the counter)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scan over the lanes of a wave
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(v, o, 64);
        if (lane >= o) v += a;
    }
    return v;
}

// column id t (0..7) of the packet words w
__device__ __forceinline__ uint32_t cell_col(const uint32_t (&w)[4], int t) { return (t & 1) ? (w[t >> 1] >> 16) : (w[t >> 1] & 0xFFFFu); }

// the raw stored values of packet p: fp32 bits, or fp16 bits in the low half (nothing for a binary index)
template <int SD>
__device__ __forceinline__ void load_raw(const void* vals, size_t p, uint32_t (&v)[8]) {
    if constexpr (SD == VS_F32) {
        const uint4 x = reinterpret_cast<const uint4*>(vals)[2 * p], y = reinterpret_cast<const uint4*>(vals)[2 * p + 1];
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
    } else if constexpr (SD == VS_F16) {
        const uint4 x = reinterpret_cast<const uint4*>(vals)[p];
        const uint32_t h[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = h[j] & 0xFFFFu;
            v[2 * j + 1] = h[j] >> 16;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = 0u;
    }
}

// ---- step (a): select -------------------------------------------------------------------------------------------------------------------------
struct SelectArgs {
    const uint32_t* pk;               // the source: [n_rows + 1], packets of 8 uint16 column ids, 8 values a packet
    const uint4* cols;
    const void* vals;
    const uint32_t* ppk;              // the protect index: row pointers and column packets (PROT)
    const uint4* pcols;
    const uint32_t* keep;             // col_keep on the device, bit c = column c may stay; null: every column
    int64_t n_rows;
    int32_t n_cols, topk;             // topk = 0: no cut
    float min_value;
    int32_t has_min;
    uint8_t* mask;                    // out: [source packets] bit t = cell t stays
    int32_t* kept;                    // out: [n_rows] cells that stay
};

// what the selection reads of a packet: the order key of every cell, which cells are eligible, which are protected
struct Cells {
    uint32_t key[8];
    uint32_t elig, prot;
};

template <int SD, bool PROT>
__device__ __forceinline__ Cells load_cells(const SelectArgs& a, size_t p, const uint32_t* keep_lds, const uint32_t* prot_lds, bool want_prot) {
    Cells c;
    const uint4 cw = a.cols[p];
    const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
    uint32_t raw[8];
    load_raw<SD>(a.vals, p, raw);
    c.elig = 0u;
    c.prot = 0u;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint32_t col = cell_col(w, t);
        const bool cell = col < (uint32_t)a.n_cols;                    // (the padding id is n_cols: padding cells are not cells)
        const uint32_t cc = cell ? col : 0u;
        float v = 1.0f;
        if constexpr (SD == VS_F32) v = __uint_as_float(raw[t]);
        if constexpr (SD == VS_F16) v = __half2float(__ushort_as_half((unsigned short)raw[t]));
        c.key[t] = SD == VS_NONE ? 0u : value_key_f32(__float_as_uint(v));
        bool ok = cell && prune_value_ok(v, a.has_min != 0, a.min_value);
        if (keep_lds) ok = ok && ((keep_lds[cc >> 5] >> (cc & 31u)) & 1u);
        c.elig |= (ok ? 1u : 0u) << t;
        if constexpr (PROT) {
            if (want_prot) c.prot |= (cell ? (prot_lds[cc >> 5] >> (cc & 31u)) & 1u : 0u) << t;
        }
    }
    return c;
}

// the wave's bitmap of the protect row's columns: set (SET = true) from the row's packets, cleared by walking the same packets again
template <bool SET>
__device__ __forceinline__ void protect_bits(const SelectArgs& a, int64_t r, uint32_t* prot_lds, int lane) {
    const uint32_t q0 = a.ppk[r], q1 = a.ppk[r + 1];
    for (uint32_t q = q0 + lane; q < q1; q += 64) {
        const uint4 cw = a.pcols[q];
        const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t col = cell_col(w, t);
            if (col < (uint32_t)a.n_cols) {
                if (SET) atomicOr(&prot_lds[col >> 5], 1u << (col & 31u));
                else prot_lds[col >> 5] = 0u;
            }
        }
    }
}

// One row by one wave.  REG: the row's packets (lane l: packets l, l + 64) are read once and held; otherwise every pass re-reads them.
template <int SD, bool PROT, bool REG>
__device__ __forceinline__ void select_row(const SelectArgs& a, int64_t r, uint32_t p0, uint32_t np, const uint32_t* keep_lds, uint32_t* hist,
                                           uint32_t* prot_lds, int lane) {
    constexpr int kUnroll = REG ? kPruneRegPackets : 1;        // (the register path's loops over a lane's packets unroll whole: reg[] is indexed statically)
    const int nj = REG ? kPruneRegPackets : (int)((np + 63u) >> 6);
    const uint32_t m = (uint32_t)a.topk;
    const bool may_cut = SD != VS_NONE && m > 0u && (uint64_t)np * 8ull > (uint64_t)m;   // (a row of at most m cells keeps its eligible cells)
    if (PROT && may_cut) {
        protect_bits<true>(a, r, prot_lds, lane);
        wave_sync();
    }
    auto load = [&](int j) -> Cells {
        const uint32_t q = (uint32_t)j * 64u + (uint32_t)lane;
        if (q < np) return load_cells<SD, PROT>(a, (size_t)p0 + q, keep_lds, prot_lds, may_cut);
        Cells c;
#pragma unroll
        for (int t = 0; t < 8; ++t) c.key[t] = 0u;
        c.elig = c.prot = 0u;
        return c;
    };
    Cells reg[REG ? kPruneRegPackets : 1];
    uint32_t n_elig = 0u;
#pragma unroll kUnroll
    for (int j = 0; j < nj; ++j) {
        const Cells c = load(j);
        if constexpr (REG) reg[j] = c;
        n_elig += __popc(c.elig);
    }
    n_elig = wave_sum(n_elig);
    auto fetch = [&](int j) -> Cells {
        if constexpr (REG) return reg[j];
        else return load(j);
    };
    const bool cut = may_cut && n_elig > m;
    uint32_t thr = 0u, need = 0u;                              // the key at rank m, and how many cells equal to it are in the top m
    if (cut) {
        uint32_t prefix = 0u, pmask = 0u;
        need = m;
        for (int round = 3; round >= 0; --round) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hist[lane * 4 + i] = 0u;
            wave_sync();
#pragma unroll kUnroll
            for (int j = 0; j < nj; ++j) {
                const Cells c = fetch(j);
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (((c.elig >> t) & 1u) && (c.key[t] & pmask) == prefix) atomicAdd(&hist[prune_digit(c.key[t], round)], 1u);
            }
            wave_sync();
            uint32_t h[4];                                     // lane l: bins 255 - 4 l down to 252 - 4 l, from the top
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = hist[255 - 4 * lane - i];
            const uint32_t s = h[0] + h[1] + h[2] + h[3];
            const uint32_t inc = wave_incl_scan(s, lane), exc = inc - s;
            const bool mine = exc < need && need <= inc;      // exactly one lane: the candidates are at least `need`
            uint32_t digit = 0u, above = 0u, acc = exc;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (mine && acc < need && need <= acc + h[i]) {
                    digit = (uint32_t)(255 - 4 * lane - i);
                    above = acc;
                }
                acc += h[i];
            }
            const unsigned long long who = __ballot(mine);
            const int from = who ? __ffsll((long long)who) - 1 : 0;
            digit = __shfl(digit, from, 64);
            above = __shfl(above, from, 64);
            need -= above;
            prefix |= digit << (8 * round);
            pmask |= 0xFFu << (8 * round);
            wave_sync();                                       // (the bins are zeroed again by the next round)
        }
        thr = prefix;
    }
    // the keep bytes: eligible and (in the top m, or protected); cells equal to the key at rank m go in stored order -- packet-major, and
    // this round's packets are the lanes' in lane order
    uint32_t eq_before = 0u, n_kept = 0u;
#pragma unroll kUnroll
    for (int j = 0; j < nj; ++j) {
        const Cells c = fetch(j);
        uint32_t kb = c.elig;
        if (cut) {
            uint32_t gt = 0u, eq = 0u;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                gt |= (c.key[t] > thr ? 1u : 0u) << t;
                eq |= (c.key[t] == thr ? 1u : 0u) << t;
            }
            gt &= c.elig;
            eq &= c.elig;
            const uint32_t cnt = __popc(eq), inc = wave_incl_scan(cnt, lane);
            const int64_t rank0 = (int64_t)eq_before + (inc - cnt);
            const int64_t left = (int64_t)need - rank0;        // cells of the tie group the top m still takes from this packet on
            const int take = left < 0 ? 0 : (left > 8 ? 8 : (int)left);
            kb = c.elig & (gt | prune_first_bits(eq, take) | c.prot);
            eq_before += __shfl(inc, 63, 64);
        }
        const uint32_t q = (uint32_t)j * 64u + (uint32_t)lane;
        if (q < np) a.mask[(size_t)p0 + q] = (uint8_t)kb;
        n_kept += __popc(kb);
    }
    n_kept = wave_sum(n_kept);
    if (lane == 0) a.kept[r] = (int32_t)n_kept;
    if (PROT && may_cut) {
        wave_sync();
        protect_bits<false>(a, r, prot_lds, lane);
        wave_sync();
    }
}

// persistent workgroups of 4 waves stride over the rows, a wave a row.  LDS: col_keep once a workgroup; a 256-bin histogram and (PROT) a
// bitmap of n_cols bits a wave
template <int SD, bool PROT>
__global__ __launch_bounds__(kPruneThreads) void prune_select_kernel(SelectArgs a) {
    extern __shared__ uint32_t prune_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int words = (a.n_cols + 31) >> 5;
    uint32_t* keep_lds = prune_lds;
    uint32_t* hist = prune_lds + words + w * kPruneBins;
    uint32_t* prot_lds = prune_lds + words + kPruneWaves * kPruneBins + (PROT ? w * words : 0);
    if (a.keep)
        for (int i = threadIdx.x; i < words; i += kPruneThreads) keep_lds[i] = a.keep[i];
    if (PROT)
        for (int i = threadIdx.x; i < kPruneWaves * words; i += kPruneThreads) prune_lds[words + kPruneWaves * kPruneBins + i] = 0u;
    __syncthreads();
    const uint32_t* keep = a.keep ? keep_lds : nullptr;
    for (int64_t r = (int64_t)blockIdx.x * kPruneWaves + w; r < a.n_rows; r += (int64_t)gridDim.x * kPruneWaves) {
        const uint32_t p0 = a.pk[r], np = a.pk[r + 1] - p0;
        if (np <= 64u * kPruneRegPackets) select_row<SD, PROT, true>(a, r, p0, np, keep, hist, prot_lds, lane);
        else select_row<SD, PROT, false>(a, r, p0, np, keep, hist, prot_lds, lane);
    }
}

// ---- step (c): pack ---------------------------------------------------------------------------------------------------------------------------
struct PackArgs {
    const uint32_t* pk;               // the source
    const uint4* cols;
    const void* vals;
    const uint8_t* mask;              // [source packets] keep bytes
    const uint32_t* new_pk;           // [n_rows + 1]
    int64_t n_rows;
    int32_t n_cols;
    uint4* dcols;                     // the new index
    void* dvals;
};

// A wave a row: the rank of a kept cell is the popcount of the keep bits before it -- a wave scan over the round's packets, the rounds before,
// the bits below it in its byte.  A source packet that stays whole and lands on a packet boundary moves as 16-byte stores; the others cell by
// cell (uint16 ids, values of the store dtype).  The tail of the row's last packet is padded with column id n_cols and value 0.
template <int SD>
__global__ __launch_bounds__(kPruneThreads) void prune_pack_kernel(PackArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint16_t* dc16 = reinterpret_cast<uint16_t*>(a.dcols);
    for (int64_t r = (int64_t)blockIdx.x * kPruneWaves + w; r < a.n_rows; r += (int64_t)gridDim.x * kPruneWaves) {
        const uint32_t s0 = a.pk[r], np = a.pk[r + 1] - s0, d0 = a.new_pk[r], nd = a.new_pk[r + 1] - d0;
        if (nd == 0u) continue;
        uint32_t before = 0u;                                  // kept cells of the rounds before
        for (uint32_t q0 = 0u; q0 < np; q0 += 64u) {
            const uint32_t q = q0 + (uint32_t)lane;
            const uint32_t b = q < np ? (uint32_t)a.mask[(size_t)s0 + q] : 0u;
            const uint32_t cnt = __popc(b), inc = wave_incl_scan(cnt, lane);
            const uint32_t rank0 = before + inc - cnt;
            before += __shfl(inc, 63, 64);
            if (b == 0u) continue;
            const size_t p = (size_t)s0 + q;
            const uint4 cw = a.cols[p];
            if (b == 0xFFu && (rank0 & 7u) == 0u) {
                const size_t d = (size_t)d0 + (rank0 >> 3);
                a.dcols[d] = cw;
                if constexpr (SD == VS_F32) {
                    const uint4* sv = reinterpret_cast<const uint4*>(a.vals);
                    uint4* dv = reinterpret_cast<uint4*>(a.dvals);
                    dv[2 * d] = sv[2 * p];
                    dv[2 * d + 1] = sv[2 * p + 1];
                }
                if constexpr (SD == VS_F16) reinterpret_cast<uint4*>(a.dvals)[d] = reinterpret_cast<const uint4*>(a.vals)[p];
                continue;
            }
            const uint32_t cwv[4] = {cw.x, cw.y, cw.z, cw.w};
            uint32_t raw[8];
            load_raw<SD>(a.vals, p, raw);
            size_t d = (size_t)d0 * 8 + rank0;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if ((b >> t) & 1u) {
                    dc16[d] = (uint16_t)cell_col(cwv, t);
                    if constexpr (SD == VS_F32) reinterpret_cast<uint32_t*>(a.dvals)[d] = raw[t];
                    if constexpr (SD == VS_F16) reinterpret_cast<uint16_t*>(a.dvals)[d] = (uint16_t)raw[t];
                    ++d;
                }
            }
        }
        const uint32_t pad = nd * 8u - before;                 // (< 8: nd = ceil(kept / 8))
        if ((uint32_t)lane < pad) {
            const size_t d = (size_t)d0 * 8 + before + (uint32_t)lane;
            dc16[d] = (uint16_t)a.n_cols;
            if constexpr (SD == VS_F32) reinterpret_cast<uint32_t*>(a.dvals)[d] = 0u;
            if constexpr (SD == VS_F16) reinterpret_cast<uint16_t*>(a.dvals)[d] = 0u;
        }
    }
}

PruneShape shape_of(const vs_index* idx) {
    PruneShape s;
    s.kind = idx->kind;
    s.store_dtype = idx->store_dtype;
    s.device = idx->device;
    s.n_rows = idx->n_rows;
    s.n_cols = idx->n_cols;
    return s;
}

template <int SD>
void launch_select(bool prot, unsigned grid, size_t lds, const SelectArgs& a) {
    if (prot) hipLaunchKernelGGL((prune_select_kernel<SD, true>), dim3(grid), dim3(kPruneThreads), lds, 0, a);
    else hipLaunchKernelGGL((prune_select_kernel<SD, false>), dim3(grid), dim3(kPruneThreads), lds, 0, a);
}

}  // namespace

extern "C" int vs_prune_plan(int64_t n_rows, int64_t n_packets, int32_t n_cols, int store_dtype, int32_t topk, int has_protect, int32_t* out_reg_cells,
                             int64_t* out_scratch_bytes, int32_t* out_lds_bytes) {
    char msg[512] = {0};
    PrunePlan p;
    const int rc = prune_plan(n_rows, n_packets, n_cols, store_dtype, topk, has_protect != 0, &p, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if (out_reg_cells) *out_reg_cells = p.reg_cells;
    if (out_scratch_bytes) *out_scratch_bytes = p.scratch_bytes;
    if (out_lds_bytes) *out_lds_bytes = p.lds_bytes;
    return VS_OK;
}

extern "C" int vs_index_prune(const vs_index* src, int32_t topk, float min_value, const uint32_t* col_keep, const vs_index* protect, int64_t rows_extra,
                              int64_t packets_extra, int device, vs_index** out, int32_t* out_kept) {
    char msg[512] = {0};
    if (out) *out = nullptr;
    const bool has_min = !std::isnan(min_value);
    int rc = new_index_check_extra(rows_extra, packets_extra, msg, sizeof msg);
    if (rc == VS_OK) rc = prune_check_rules(topk, has_min, src ? src->store_dtype : VS_F32, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if (!src || !out) return fail(VS_EINVAL, "NULL argument");
    rc = prune_check_source(shape_of(src), msg, sizeof msg);
    if (rc == VS_OK && protect) rc = prune_check_protect(shape_of(src), shape_of(protect), msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(device_in_range(device));
    const bool keep_dev = is_device_ptr(col_keep), kept_dev = is_device_ptr(out_kept);
    rc = prune_check_pointers(col_keep != nullptr, keep_dev, out_kept != nullptr, kept_dev, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(ptr_on(col_keep, keep_dev, src->device, "col_keep"));
    VS_TRY(ptr_on(out_kept, kept_dev, src->device, "out_kept"));
    PrunePlan plan;
    rc = prune_plan(src->n_rows, src->n_packets, src->n_cols, src->store_dtype, topk, protect != nullptr, &plan, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);

    VS_TRY(open_sources(src->device));
    const int64_t n = src->n_rows, n_src_packets = src->n_packets;
    const int sd = src->store_dtype;
    // scratch: keep bytes, kept counts, block sums, the non-zero count
    DevBuf mask, kept_buf, sums, cnt, keep_stage;
    if (mask.alloc((size_t)n_src_packets) != VS_OK)
        return fail(VS_ENOMEM, "pruning needs %lld bytes of HBM for the keep bytes of the source's packets", (long long)n_src_packets);
    int32_t* d_kept = out_kept;
    if (!kept_dev) {
        VS_TRY(kept_buf.alloc(std::max<size_t>((size_t)n * 4, 4)));
        d_kept = kept_buf.as<int32_t>();
    }
    VS_TRY(sums.alloc((size_t)(plan.scan_blocks + 1) * 8));
    VS_TRY(cnt.alloc(8));
    VS_HIP(hipMemset(cnt.p, 0, 8));
    const void* d_keep = nullptr;
    if (col_keep) VS_TRY(to_device(col_keep, (size_t)prune_keep_words(src->n_cols) * 4, keep_stage, 0, &d_keep));
    // (a) select
    if (n > 0) {
        SelectArgs a;
        a.pk = src->pk_ptr.as<uint32_t>();
        a.cols = src->cols.as<uint4>();
        a.vals = src->vals.p;
        a.ppk = protect ? protect->pk_ptr.as<uint32_t>() : nullptr;
        a.pcols = protect ? protect->cols.as<uint4>() : nullptr;
        a.keep = (const uint32_t*)d_keep;
        a.n_rows = n;
        a.n_cols = src->n_cols;
        a.topk = topk;
        a.min_value = has_min ? min_value : 0.f;
        a.has_min = has_min ? 1 : 0;
        a.mask = mask.as<uint8_t>();
        a.kept = d_kept;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kPruneWaves - 1) / kPruneWaves, (int64_t)src->cu_count * 8));
        if (sd == VS_F32) launch_select<VS_F32>(protect != nullptr, grid, (size_t)plan.lds_bytes, a);
        else if (sd == VS_F16) launch_select<VS_F16>(protect != nullptr, grid, (size_t)plan.lds_bytes, a);
        else launch_select<VS_NONE>(protect != nullptr, grid, (size_t)plan.lds_bytes, a);
        VS_HIP(hipGetLastError());
    }
    // (b) scan
    uint2* d_sums = sums.as<uint2>();
    int64_t p_new = 0;
    VS_TRY(cells_scan(d_kept, n, plan.scan_blocks, d_sums, cnt.as<unsigned long long>(), &p_new));
    unsigned long long nnz = 0;
    VS_HIP(hipMemcpy(&nnz, cnt.p, 8, hipMemcpyDeviceToHost));
    rc = new_index_check_capacity("pruned", n, p_new, rows_extra, packets_extra, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    IndexGuard guard{nullptr};
    VS_TRY(new_csr_index("pruning", "source's (drop the postings copy of the source, or prune onto fewer cells)", n, p_new, rows_extra, packets_extra, src->n_cols,
                         sd, src->device, &guard));
    vs_index* idx = guard.p;
    VS_TRY(cells_row_pointers(d_kept, n, plan.scan_blocks, d_sums, p_new, idx->pk_ptr.as<uint32_t>()));
    // (c) pack
    if (p_new > 0) {
        PackArgs a;
        a.pk = src->pk_ptr.as<uint32_t>();
        a.cols = src->cols.as<uint4>();
        a.vals = src->vals.p;
        a.mask = mask.as<uint8_t>();
        a.new_pk = idx->pk_ptr.as<uint32_t>();
        a.n_rows = n;
        a.n_cols = src->n_cols;
        a.dcols = idx->cols.as<uint4>();
        a.dvals = idx->vals.p;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kPruneWaves - 1) / kPruneWaves, (int64_t)src->cu_count * 16));
        if (sd == VS_F32) hipLaunchKernelGGL(prune_pack_kernel<VS_F32>, dim3(grid), dim3(kPruneThreads), 0, 0, a);
        else if (sd == VS_F16) hipLaunchKernelGGL(prune_pack_kernel<VS_F16>, dim3(grid), dim3(kPruneThreads), 0, 0, a);
        else hipLaunchKernelGGL(prune_pack_kernel<VS_NONE>, dim3(grid), dim3(kPruneThreads), 0, 0, a);
        VS_HIP(hipGetLastError());
    }
    set_csr_shape(idx, n, p_new, (int64_t)nnz, src->logical_dense);
    if (out_kept && !kept_dev && n > 0) VS_HIP(hipMemcpy(out_kept, d_kept, (size_t)n * 4, hipMemcpyDeviceToHost));
    return hand_over(guard, src->device, device, TombFrom::source_bits(src), out);
}
