// agg_call.h -- the host side every aggregation call shares (facets, term counts, term sums, numeric fields, percentiles): the small helpers of
// an entry point, staging a set's bitmaps, the [B, n] int64 matrix + [B] vectors output pattern, the launch ladder over an index's store dtype,
// and the kernel arguments of the term aggregations.  The buffers of a call follow staging.h: all host (staged, copied back, the call blocks)
// or all device (only enqueued).
#pragma once
#include "common.h"
#include "packets.h"
#include "staging.h"
#include "term_agg_check.h"

#include <initializer_list>
#include <type_traits>

namespace vs {

inline int plan_or_fail(int rc, const char* msg) { return rc == VS_OK ? VS_OK : fail(rc, "%s", msg); }

inline int device_in_range(int device) {
    VS_TRY(need_device());
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    return VS_OK;
}

inline int finish_call(bool dev, void* stream, hipStream_t s) {
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

// a failed launch ends the call: the staging buffers die with it, so the stream is drained first
inline int launch_rc(int rc, hipStream_t s) {
    if (rc != VS_OK) (void)hipStreamSynchronize(s);
    return rc;
}

// tombstones are ANDed in, as every search does (the live bitmap starts at bit 0 whatever bit0 is)
inline const uint32_t* live_words(vs_index* idx) { return idx->has_tomb ? idx->live.as<uint32_t>() : nullptr; }

// what: "term counts" | "term sums"
inline int csr_index_ok(const vs_index* idx, const char* what) {
    if (idx->kind != VS_KIND_CSR) return fail(VS_EUNSUPPORTED, "%s read the CSR packets: a dense index on the matrix cores has none", what);
    if (idx->n_cols > kTermMaxCols) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", idx->n_cols);
    return VS_OK;
}

// The staged bitmaps of a set.  and_user: a caller's second bitmap (of the kind of the other pointers, at bit0); and_dev: a device bitmap at
// bit 0 (an index's live rows).  At most one of the two.
struct BitmapStage {
    Staged w, a;
    int in(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_user, const uint32_t* and_dev, int32_t B, int64_t n_rows,
           int64_t rows_per_chunk, bool dev, hipStream_t s, RowSet* out) {
        const int64_t span = (bit0 + n_rows + 31) >> 5;
        uint32_t *d_w, *d_a;
        VS_TRY(w.in(words, (size_t)((B - 1) * ld_words + span), dev, true, s, &d_w));
        VS_TRY(a.in(and_user, (size_t)span, dev, true, s, &d_a));
        out->words = d_w;
        out->bit0 = bit0;
        out->ld_words = words ? ld_words : 0;
        out->and_words = and_user ? d_a : and_dev;
        out->and_bit0 = and_user ? bit0 : 0;
        out->n_rows = n_rows;
        out->B = B;
        out->rows_per_chunk = rows_per_chunk;
        return VS_OK;
    }
};

// a set with one 32-bit value a row: the kernel arguments and the staging of the numeric fields (values.hip, quantiles.hip)
struct SetArgs {
    RowSet set;
    const uint32_t* values;           // [n_rows] raw
    int dtype;
};
struct SetStage {
    BitmapStage b;
    Staged v;
    int in(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_user, const uint32_t* and_dev, int32_t B, const void* values,
           int dtype, int64_t n_rows, int64_t rows_per_chunk, bool dev, hipStream_t s, SetArgs* out) {
        VS_TRY(b.in(words, bit0, ld_words, and_user, and_dev, B, n_rows, rows_per_chunk, dev, s, &out->set));
        uint32_t* d_v;
        VS_TRY(v.in(static_cast<const uint32_t*>(values), (size_t)n_rows, dev, true, s, &d_v));
        out->values = d_v;
        out->dtype = dtype;
        return VS_OK;
    }
};

// The outputs of a counting call: an int64 matrix [B, n] of stride ld and up to three int64 vectors [B], all zero before the kernel adds to
// them.  Device outputs are zeroed in place; host outputs get one zeroed device buffer (the matrix dense, the vectors behind it) that back()
// copies out.
struct CountsOut {
    DevBuf buf;
    unsigned long long* mat = nullptr;
    int64_t ld = 0;
    unsigned long long* vec[3] = {};
    int bind(bool dev, int64_t* u_mat, int64_t u_ld, int64_t n, int32_t B, std::initializer_list<int64_t*> u_vecs, hipStream_t s) {
        n_ = n, B_ = B, u_mat_ = u_mat, u_ld_ = u_ld, nv_ = 0;
        for (int64_t* v : u_vecs) u_vec_[nv_++] = v;
        const size_t n_mat = (size_t)B * (size_t)n;
        if (dev) {
            mat = reinterpret_cast<unsigned long long*>(u_mat);
            ld = u_ld;
            if (u_ld == n || B == 1) VS_HIP(hipMemsetAsync(mat, 0, n_mat * 8, s));
            else VS_HIP(hipMemset2DAsync(mat, (size_t)u_ld * 8, 0, (size_t)n * 8, (size_t)B, s));
            for (int i = 0; i < nv_; ++i) {
                vec[i] = reinterpret_cast<unsigned long long*>(u_vec_[i]);
                VS_HIP(hipMemsetAsync(vec[i], 0, (size_t)B * 8, s));
            }
        } else {
            VS_TRY(buf.alloc((n_mat + (size_t)nv_ * (size_t)B) * 8));
            mat = buf.as<unsigned long long>();
            ld = n;
            for (int i = 0; i < nv_; ++i) vec[i] = mat + n_mat + (size_t)i * (size_t)B;
            VS_HIP(hipMemsetAsync(buf.p, 0, buf.bytes, s));
        }
        return VS_OK;
    }
    // host outputs only
    int back(hipStream_t s) {
        VS_HIP(hipMemcpy2DAsync(u_mat_, (size_t)u_ld_ * 8, mat, (size_t)n_ * 8, (size_t)n_ * 8, (size_t)B_, hipMemcpyDeviceToHost, s));
        for (int i = 0; i < nv_; ++i) VS_HIP(hipMemcpyAsync(u_vec_[i], vec[i], (size_t)B_ * 8, hipMemcpyDeviceToHost, s));
        return VS_OK;
    }

private:
    int64_t n_ = 0, u_ld_ = 0;
    int32_t B_ = 0;
    int nv_ = 0;
    int64_t *u_mat_ = nullptr, *u_vec_[3] = {};
};

// f(SD, IDS) as std::integral_constants, for the store dtype of an index -- VS_F32 | VS_F16 | VS_NONE (a binary index) -- and the kind of the
// set: the six kernels of a term aggregation
template <class F>
int dispatch_store(int sd, bool ids, F f) {
    auto with = [&](auto SD) { return ids ? f(SD, std::integral_constant<int, 1>{}) : f(SD, std::integral_constant<int, 0>{}); };
    if (sd == VS_F32) return with(std::integral_constant<int, VS_F32>{});
    if (sd == VS_F16) return with(std::integral_constant<int, VS_F16>{});
    return with(std::integral_constant<int, VS_NONE>{});
}

// The set of a term aggregation on the index's device -- (words, bit0, ld_words) when ids == nullptr, else the id lists -- staged and written
// into *a.  A host id list under strict is checked first: every id is -1 or names a row of the index.
struct TermStage {
    Staged w, i;
    int in(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, const int64_t* ids, int64_t m, int64_t ld_ids, int64_t id_offset,
           int strict, int32_t B, int64_t rows_per_chunk, bool dev, hipStream_t s, TermSetArgs* a) {
        if (ids && !dev && strict) {
            char msg[256];
            VS_TRY(plan_or_fail(term_check_ids_host(ids, B, m, ld_ids, id_offset, idx->n_rows, msg, sizeof msg), msg));
        }
        VS_HIP(hipSetDevice(idx->device));
        uint32_t* d_w = nullptr;
        int64_t* d_i = nullptr;
        if (ids) {
            VS_TRY(i.in(ids, (size_t)(B - 1) * (size_t)ld_ids + (size_t)m, dev, true, s, &d_i));
        } else {
            const int64_t span = (bit0 + idx->n_rows + 31) >> 5;
            VS_TRY(w.in(words, (size_t)((B - 1) * ld_words + span), dev, true, s, &d_w));
        }
        a->pk_ptr = idx->pk_ptr.as<uint32_t>();
        a->cols = idx->cols.as<uint4>();
        a->vals = idx->vals.p;
        a->n_cols = idx->n_cols;
        a->set = RowSet{d_w, bit0, words ? ld_words : 0, live_words(idx), 0, idx->n_rows, B, rows_per_chunk};
        a->ids = d_i;
        a->ld_ids = ld_ids;
        a->m = m;
        a->id_offset = id_offset;
        return VS_OK;
    }
};

// One [B, n_cols] term aggregation on the index's device: pointer kinds, the set, the outputs, launch(SD, IDS, set, out) -> code on the stream
// (dispatch_store's constants; skipped for an index without rows), and the way back.  names: the call's words for its matrix and for the profile ("counts",
// "term_counts").
template <class Launch>
int term_agg_call(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, const int64_t* ids, int64_t m, int64_t ld_ids,
                  int64_t id_offset, int strict, int32_t B, int64_t rows_per_chunk, const char* out_name, const char* prof_name, int64_t* out,
                  int64_t ld_out, int64_t* total, void* stream, Launch launch) {
    const void* ptrs[4] = {words, ids, out, total};
    const char* names[4] = {"words", "ids", out_name, "total"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 4, idx->device, &dev));
    hipStream_t s = (hipStream_t)stream;
    TermStage st;
    CountsOut o;
    TermSetArgs a{};
    VS_TRY(st.in(idx, words, bit0, ld_words, ids, m, ld_ids, id_offset, strict, B, rows_per_chunk, dev, s, &a));
    VS_TRY(o.bind(dev, out, ld_out, idx->n_cols, B, {total}, s));
    if (idx->n_rows > 0) {
        ProfScope prof(prof_name, s);
        VS_TRY(launch_rc(dispatch_store(idx->store_dtype, ids != nullptr, [&](auto sd, auto is_ids) { return launch(sd, is_ids, a, o); }), s));
    }
    VS_STAGE(prof_name, s);
    if (!dev) VS_TRY(o.back(s));
    return finish_call(dev, stream, s);
}

}  // namespace vs
