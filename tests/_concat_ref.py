"""numpy reference of the joined index (the contract is pinned in include/vsearch_hip.h: vs_index_concat) on exported CSR.

A source is (indptr, indices, data): data float32 -- the stored values widened exactly, as export_csr returns them -- or None for a binary
(bag-of-token) source.  The result's store is "fp32", "fp16" or "binary"; its data is float32 again (the fp16 values widened), so that every
comparison is on float32 BITS.  The fp32 -> fp16 rounding is written out on the bits (round to nearest, ties to even) and pinned against numpy's
by tests/test_concat_cpu.py."""
import numpy as np

STORES = ("fp32", "fp16", "binary")


def f16_bits(x):
    """float32 array -> the uint16 bits of the nearest float16, ties to even: overflow gives +-inf, results below the smallest normal are
    subnormal (never flushed), a NaN gives the quiet NaN of its sign"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    sign = (b >> np.uint64(16)) & np.uint64(0x8000)
    e = ((b >> np.uint64(23)) & np.uint64(0xFF)).astype(np.int64)
    m = b & np.uint64(0x7FFFFF)
    E = e - 127 + 15                                            # the float16 exponent field of a normal result
    # a normal result: 10 of the 23 mantissa bits stay; a carry out of the mantissa goes into the exponent (up to the bits of inf)
    h = (np.clip(E, 0, 31).astype(np.uint64) << np.uint64(10)) | (m >> np.uint64(13))
    rem = m & np.uint64(0x1FFF)
    up = (rem > np.uint64(0x1000)) | ((rem == np.uint64(0x1000)) & ((h & np.uint64(1)) == np.uint64(1)))
    normal = h + up.astype(np.uint64)
    # a subnormal result: the 24-bit significand shifted down to units of 2^-24
    full = m | np.uint64(0x800000)
    shift = np.clip(14 - E, 1, 40).astype(np.uint64)
    hs = full >> shift
    rem = full & ((np.uint64(1) << shift) - np.uint64(1))
    half = np.uint64(1) << (shift - np.uint64(1))
    sub = hs + ((rem > half) | ((rem == half) & ((hs & np.uint64(1)) == np.uint64(1)))).astype(np.uint64)
    out = np.where(E >= 1, normal, sub)
    out = np.where(e == 0, np.uint64(0), out)                   # a float32 zero or subnormal is far below 2^-25
    out = np.where(E >= 31, np.uint64(0x7C00), out)             # beyond the range (and every float32 inf)
    out = np.where((e == 255) & (m != 0), np.uint64(0x7E00), out)
    return (out | sign).astype(np.uint16)


def to_f16(x):
    """float32 array -> the float32 values a float16 store holds of it"""
    return f16_bits(x).view(np.float16).astype(np.float32)


def default_store(stores):
    """the store concat(dtype=None) picks: binary if every source is, fp16 if every valued source is fp16, else fp32"""
    valued = [s for s in stores if s != "binary"]
    if not valued:
        return "binary"
    return "fp16" if all(s == "fp16" for s in valued) else "fp32"


def convert(data, nnz, out):
    """the values of one source in the result's store (float32, the fp16 ones widened); None for a binary result"""
    if out == "binary":
        if data is not None:
            raise ValueError("binarising is not covered")
        return None
    v = np.ones(nnz, dtype=np.float32) if data is None else np.ascontiguousarray(data, dtype=np.float32)
    return to_f16(v) if out == "fp16" else v


def concat_ref(sources, out):
    """sources: a list of (indptr, indices, data | None); out: the result's store -> (indptr int64, indices int64, data float32 | None)"""
    if out not in STORES:
        raise ValueError(f"bad store {out!r}")
    if not sources:
        raise ValueError("no sources")
    ips, ixs, ds, base = [np.zeros(1, np.int64)], [], [], 0
    for ip, ix, d in sources:
        ip = np.asarray(ip, dtype=np.int64)
        ips.append(ip[1:] + base)                               # row pointer R_s + r = the source's + the cells before it
        base += int(ip[-1])
        ixs.append(np.asarray(ix, dtype=np.int64)[:int(ip[-1])])
        ds.append(convert(d, int(ip[-1]), out))
    ip = np.concatenate(ips)
    if len(ip) == 1:
        raise ValueError("empty join")
    return ip, np.concatenate(ixs), (None if out == "binary" else np.concatenate(ds).astype(np.float32))


def concat_live(masks):
    """the live mask of the result: the sources' masks one behind the other (a result row is deleted iff its source row is)"""
    return np.concatenate([np.asarray(m, dtype=bool) for m in masks])


def packets_of(indptr):
    """the 8-cell packets of a CSR's rows"""
    return int(((np.diff(np.asarray(indptr, dtype=np.int64)) + 7) // 8).sum())


def rebased_packet_pointers(indptrs):
    """the row pointers of the device format, in packets: new pointer R_s + r = src_pk_s[r] + P_s, the last one the packet total"""
    out, base = [], 0
    for ip in indptrs:
        pk = np.concatenate([[0], np.cumsum((np.diff(np.asarray(ip, dtype=np.int64)) + 7) // 8)])
        out.append(pk[:-1] + base)
        base += int(pk[-1])
    return np.concatenate(out + [[base]]).astype(np.int64)


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and ((a[2] is None and b[2] is None) or same_bits(a[2], b[2]))
