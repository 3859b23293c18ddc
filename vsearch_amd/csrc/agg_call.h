// agg_call.h -- the host side every aggregation call shares (facets, term counts, term sums, numeric fields, percentiles): the small helpers of
// an entry point, the opening and the tail of a call, where a call's set lives (SetSrc: the free form's arguments, or an index) and the staging
// of its bitmaps, the [B, n] int64 matrix + [B] vectors output pattern, the launch ladders over a plan's query tile and an index's store dtype,
// and the kernel arguments of the term aggregations.  The buffers of a call follow staging.h: all host (staged, copied back, the call blocks)
// or all device (only enqueued).  An aggregation over a bitmap set is a kernel body, a check, one body function over a SetSrc and two
// extern "C" wrappers.
#pragma once
#include "common.h"
#include "packets.h"
#include "staging.h"
#include "term_agg_check.h"

#include <initializer_list>
#include <type_traits>

namespace vs {

inline int plan_or_fail(int rc, const char* msg) { return rc == VS_OK ? VS_OK : fail(rc, "%s", msg); }

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

// the launches of a call, looked at once they are all enqueued: "<name> launch failed: <hip string>"
inline int launch_failed(const char* name, hipStream_t s) {
    const hipError_t le = hipGetLastError();
    if (le == hipSuccess) return VS_OK;
    (void)hipStreamSynchronize(s);                                  // staging buffers and scratch die with the caller
    return fail(VS_EHIP, "%s launch failed: %s", name, hipGetErrorString(le));
}

// how a call ends: kStream as finish_call does (device buffers on a stream: only enqueued); kSync always synchronises, for a call that owns
// scratch the kernels use (it is freed when the call returns)
enum class Finish { kStream, kSync };

// The tail of a call, once everything is enqueued: the look at the launches, the stage mark, back() -> code (the copies to host buffers) and
// the finish.
template <class Back>
int close_call(const char* name, bool dev, void* stream, hipStream_t s, Finish fin, Back back) {
    VS_TRY(launch_failed(name, s));
    VS_STAGE(name, s);
    if (!dev) VS_TRY(launch_rc(back(), s));
    if (fin == Finish::kStream) return finish_call(dev, stream, s);
    VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

// The opening of a call: its buffers are all host or all device pointers on `device` (-> dev), the device is set, the stream cast.
struct NamedPtr {
    const char* name;
    const void* p;
};
struct Call {
    bool dev = false;
    void* stream = nullptr;
    hipStream_t s = nullptr;
    int open(int device, void* stream_, std::initializer_list<NamedPtr> bufs) {
        const void* ptrs[16];
        const char* names[16];
        int n = 0;
        for (const NamedPtr& b : bufs) {
            if (n == 16) return fail(VS_EINVAL, "too many buffers in one call");
            names[n] = b.name;
            ptrs[n++] = b.p;
        }
        VS_TRY(pointers_kind(ptrs, names, n, device, &dev));
        VS_HIP(hipSetDevice(device));
        stream = stream_;
        s = (hipStream_t)stream_;
        return VS_OK;
    }
    // enqueue() -> code stages, zeroes and launches; whatever it returns early with, the stream is drained before the call's buffers die
    template <class Enqueue, class Back>
    int run(const char* name, Finish fin, Enqueue enqueue, Back back) {
        VS_TRY(launch_rc(enqueue(), s));
        return close_call(name, dev, stream, s, fin, back);
    }
};

// f(QT) as a std::integral_constant for the query tile of a plan: 8 | 4 | 2 | 1
template <class F>
int launch_by_qt(int qt, F f) {
    if (qt == 8) return f(std::integral_constant<int, 8>{});
    if (qt == 4) return f(std::integral_constant<int, 4>{});
    if (qt == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 1>{});
}

// tombstones are ANDed in, as every search does (the live bitmap starts at bit 0 whatever bit0 is)
inline const uint32_t* live_words(vs_index* idx) { return idx->has_tomb ? idx->live.as<uint32_t>() : nullptr; }

// what: "term counts" | "term sums"
inline int csr_index_ok(const vs_index* idx, const char* what) {
    if (idx->kind != VS_KIND_CSR) return fail(VS_EUNSUPPORTED, "%s read the CSR packets: a dense index on the matrix cores has none", what);
    if (idx->n_cols > kTermMaxCols) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", idx->n_cols);
    return VS_OK;
}

// Where the set of a call lives: the packed bitmaps, the rows behind them and the device.  The second bitmap ANDed in is a caller's and_user
// (of the kind of the other pointers, at bit0) or a device and_dev at bit 0 (an index's live rows): at most one of the two.
struct SetSrc {
    const uint32_t* words = nullptr;
    int64_t bit0 = 0, ld_words = 0;
    int32_t B = 0;
    int64_t n_rows = 0;
    int device = 0;
    const uint32_t *and_user = nullptr, *and_dev = nullptr;
    bool free_form = false;           // the device is the caller's word and still unchecked
    bool per_query() const { return words && ld_words != 0; }
    // after the device-free argument checks, before any pointer is looked at
    int device_ok() const { return free_form ? device_in_range(device) : VS_OK; }
};
// the free form: vs_X(words, ..., and_words, ..., n_rows, ..., device)
inline SetSrc free_set(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows, int device) {
    SetSrc r;
    r.words = words, r.bit0 = bit0, r.ld_words = ld_words, r.B = B, r.n_rows = n_rows, r.device = device;
    r.and_user = and_words;
    r.free_form = true;
    return r;
}
// the index-bound form: vs_index_X(idx, words, ...) -- the index's rows on its device, its live rows ANDed in
inline SetSrc index_set(vs_index& idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B) {
    SetSrc r;
    r.words = words, r.bit0 = bit0, r.ld_words = ld_words, r.B = B, r.n_rows = idx.n_rows, r.device = idx.device;
    r.and_dev = live_words(&idx);
    return r;
}
inline int index_set(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, SetSrc* out) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    *out = index_set(*idx, words, bit0, ld_words, B);
    return VS_OK;
}

// The staged bitmaps of a set.
struct BitmapStage {
    Staged w, a;
    int in(const SetSrc& src, int64_t rows_per_chunk, bool dev, hipStream_t s, RowSet* out) {
        const int64_t span = (src.bit0 + src.n_rows + 31) >> 5;
        uint32_t *d_w, *d_a;
        VS_TRY(w.in(src.words, (size_t)((src.B - 1) * src.ld_words + span), dev, true, s, &d_w));
        VS_TRY(a.in(src.and_user, (size_t)span, dev, true, s, &d_a));
        out->words = d_w;
        out->bit0 = src.bit0;
        out->ld_words = src.words ? src.ld_words : 0;
        out->and_words = src.and_user ? d_a : src.and_dev;
        out->and_bit0 = src.and_user ? src.bit0 : 0;
        out->n_rows = src.n_rows;
        out->B = src.B;
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
    int in(const SetSrc& src, const void* values, int dtype, int64_t rows_per_chunk, bool dev, hipStream_t s, SetArgs* out) {
        VS_TRY(b.in(src, rows_per_chunk, dev, s, &out->set));
        uint32_t* d_v;
        VS_TRY(v.in(static_cast<const uint32_t*>(values), (size_t)src.n_rows, dev, true, s, &d_v));
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
    return close_call(prof_name, dev, stream, s, Finish::kStream, [&] { return o.back(s); });
}

}  // namespace vs
