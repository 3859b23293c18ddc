// set_walk.h -- how a workgroup's waves walk a document set: the three walks every aggregation shares, as templates that take
// the kernel's body as a callable (inlined: no scratch, no call).
//   walk_tile  a wave per span, a tile of QT queries: facet counts, value stats / histogram / radix counts
//   walk_rows  every wave on the same span, its 64-row steps dealt out, one query: term counts, term sums, value top-k
//   walk_ids   an id list, 64 entries a wave: term counts, term sums
// A bitmap is walked in spans of kSpanRows rows (bitmap_span.h): lane l holds words l and l + 1, so the 64 bits of any 64-row step come out of
// three lane reads whatever bit the rows start at.  A span whose words -- the set's or the and-bitmap's -- are all zero is left at once, a step
// without a set row is skipped.
#pragma once
#include "bitmap_span.h"
#include "set_check.h"

namespace vs {

static_assert(kSpanRows == 64 * 32, "load_span: a lane holds two words of a span");

// the rows of a call and the sets over them
struct RowSet {
    const uint32_t* words;            // [B, ld_words] or null (every row set)
    int64_t bit0, ld_words;
    const uint32_t* and_words;        // shared by the queries (a caller's second bitmap, an index's live rows), or null
    int64_t and_bit0;
    int64_t n_rows;
    int32_t B;
    int64_t rows_per_chunk;
};

// bits at or past the last of nvalid (>= 1) rows are ignored
__device__ __forceinline__ uint64_t valid_mask(int64_t nvalid) { return nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1ull); }

// One wave's walk over its spans of rows [r0, r1) for queries q0 .. q0 + nq - 1 (nq <= QT): body(row0, many, sp, s, sh, live) is called for
// every 64-row step with a set row.  many: the rows some query of the tile has -- the body loads its payload under (many >> lane) & 1, once
// for the tile; query q's rows of the step are window64(sp[q], s, sh) & live.
template <int QT, int WAVES, class Body>
__device__ __forceinline__ void walk_tile(const RowSet& a, int q0, int nq, int64_t r0, int64_t r1, int w, int lane, Body body) {
    const int64_t n_w = (a.bit0 + a.n_rows + 31) >> 5, n_aw = (a.and_bit0 + a.n_rows + 31) >> 5;
    for (int64_t rb = r0 + (int64_t)w * kSpanRows; rb < r1; rb += (int64_t)WAVES * kSpanRows) {
        const int nsub = (int)((min(r1, rb + kSpanRows) - rb + 63) >> 6);
        Span an{~0u, ~0u};
        int sha = 0;
        if (a.and_words) {
            const int64_t p = a.and_bit0 + rb;
            an = load_span(a.and_words, p >> 5, n_aw, lane);
            sha = (int)(p & 31);
            if (__builtin_amdgcn_ballot_w64((an.lo | an.hi) != 0u) == 0ull) continue;
        }
        Span sp[QT];
        Span u{~0u, ~0u};
        int sh = 0;
        if (a.words) {
            const int64_t p = a.bit0 + rb;
            sh = (int)(p & 31);
            u.lo = u.hi = 0u;
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                sp[q] = Span{0u, 0u};
                if (q < nq) sp[q] = load_span(a.words + (size_t)(q0 + q) * (size_t)a.ld_words, p >> 5, n_w, lane);
                u.lo |= sp[q].lo;
                u.hi |= sp[q].hi;
            }
            if (__builtin_amdgcn_ballot_w64((u.lo | u.hi) != 0u) == 0ull) continue;      // no row of the span is touched
        } else {
#pragma unroll
            for (int q = 0; q < QT; ++q) sp[q] = u;
        }
        for (int s = 0; s < nsub; ++s) {
            const int64_t row0 = rb + (int64_t)s * 64;
            const uint64_t live = window64(an, s, sha) & valid_mask(r1 - row0);
            const uint64_t many = window64(u, s, sh) & live;
            if (many == 0ull) continue;                                              // (uniform)
            body(row0, many, sp, s, sh, live);
        }
    }
}

// A workgroup's walk over rows [r0, r1) for query b: every wave loads the words of the same span, so that the decision to leave a span is
// uniform over the workgroup, and takes every WAVES-th of its 64-row steps.  body(row0, m, nvalid) is called for every step with a set row
// (m: its rows; nvalid >= 1: the rows from row0 to r1); after_span() runs once on every wave after each span that was not left
// -- a kernel's barrier goes there.
template <int WAVES, class Body, class After>
__device__ __forceinline__ void walk_rows(const RowSet& a, size_t b, int64_t r0, int64_t r1, int w, int lane, Body body, After after_span) {
    const int64_t n_w = (a.bit0 + a.n_rows + 31) >> 5, n_aw = (a.and_bit0 + a.n_rows + 31) >> 5;
    const uint32_t* wq = a.words ? a.words + b * (size_t)a.ld_words : nullptr;
    for (int64_t rb = r0; rb < r1; rb += kSpanRows) {
        const int nsub = (int)((min(r1, rb + kSpanRows) - rb + 63) >> 6);
        Span an{~0u, ~0u}, sp{~0u, ~0u};
        int sha = 0, sh = 0;
        if (a.and_words) {
            const int64_t p = a.and_bit0 + rb;
            an = load_span(a.and_words, p >> 5, n_aw, lane);
            sha = (int)(p & 31);
            if (__builtin_amdgcn_ballot_w64((an.lo | an.hi) != 0u) == 0ull) continue;
        }
        if (wq) {
            const int64_t p = a.bit0 + rb;
            sp = load_span(wq, p >> 5, n_w, lane);
            sh = (int)(p & 31);
            if (__builtin_amdgcn_ballot_w64((sp.lo | sp.hi) != 0u) == 0ull) continue;
        }
        for (int s = w; s < nsub; s += WAVES) {
            const int64_t row0 = rb + (int64_t)s * 64;
            const int64_t nvalid = r1 - row0;                                        // >= 1
            const uint64_t m = window64(an, s, sha) & window64(sp, s, sh) & valid_mask(nvalid);
            if (m == 0ull) continue;                                                 // (uniform) no row is touched
            body(row0, m, nvalid);
        }
        after_span();
    }
}

// The set rows of a step (mask m; lane l holds [plo, phi) of row l: its packets) fall into runs of consecutive rows, and the packets of a run
// are one contiguous range: f(p0, p1) once a run.
template <class F>
__device__ __forceinline__ void for_each_run(uint64_t m, uint32_t plo, uint32_t phi, F f) {
    while (m) {
        const int first = __builtin_ctzll(m);
        const uint64_t up = ~(m >> first);                                           // (bit `len` is the first clear one behind the run)
        const int len = up ? __builtin_ctzll(up) : 64;
        const int last = first + len - 1;                                            // <= 63
        f((uint32_t)__builtin_amdgcn_readlane((int)plo, first), (uint32_t)__builtin_amdgcn_readlane((int)phi, last));
        m = last >= 63 ? 0ull : (m & (~0ull << (last + 1)));
    }
}

// walk_rows over rows that are ranges of a pointer array (pk_ptr [n_rows + 1]): on_packets(p0, p1) once a run of set rows -> the set rows seen
// (wave-uniform: a chunk holds fewer than 2^32 rows)
template <int WAVES, class F>
__device__ __forceinline__ uint32_t walk_row_packets(const RowSet& a, size_t b, int64_t r0, int64_t r1, const uint32_t* pk_ptr, int w, int lane,
                                                     F on_packets) {
    uint32_t tot = 0u;
    walk_rows<WAVES>(a, b, r0, r1, w, lane, [&](int64_t row0, uint64_t m, int64_t nvalid) {
        tot += (uint32_t)__popcll(m);
        uint32_t plo = 0u, phi = 0u;
        if (lane < nvalid) {
            plo = pk_ptr[row0 + lane];
            phi = pk_ptr[row0 + lane + 1];
        }
        for_each_run(m, plo, phi, on_packets);
    }, [] {});
    return tot;
}

// A workgroup's walk over entries [e0, e1) of an id list: a wave takes 64 entries, each lane resolves its id (-1, outside [id_offset, id_offset +
// n_rows), deleted in `live`: skipped), and on_packets(p0, p1) is called for the surviving rows one after the other -> the rows seen (an id
// listed twice counts twice).
template <int WAVES, class F>
__device__ __forceinline__ uint32_t walk_ids(const int64_t* list, int64_t e0, int64_t e1, int64_t id_offset, int64_t n_rows, const uint32_t* live,
                                             const uint32_t* pk_ptr, int w, int lane, F on_packets) {
    uint32_t tot = 0u;
    for (int64_t eb = e0 + (int64_t)w * 64; eb < e1; eb += (int64_t)WAVES * 64) {
        const int64_t e = eb + lane;
        bool ok = false;
        uint32_t plo = 0u, phi = 0u;
        if (e < e1) {
            const int64_t id = list[e];
            const uint64_t row = (uint64_t)id - (uint64_t)id_offset;
            ok = id != -1 && id >= id_offset && row < (uint64_t)n_rows;              // anything else is not this index's: skipped
            if (ok && live) ok = ((live[row >> 5] >> (row & 31u)) & 1u) != 0u;       // a deleted row is skipped
            if (ok) {
                plo = pk_ptr[row];
                phi = pk_ptr[row + 1];
            }
        }
        unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        tot += (uint32_t)__popcll(m);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            on_packets((uint32_t)__builtin_amdgcn_readlane((int)plo, l), (uint32_t)__builtin_amdgcn_readlane((int)phi, l));
        }
    }
    return tot;
}

}  // namespace vs
