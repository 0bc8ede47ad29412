// Fixed-base columns (fixed_base.hpp): table construction with a device-side "same base as last time?" check, and
// the table-driven evaluation kernels (one base per column, and per-lane sums over a set of bases, in G1 and in G2).
// The cache protocol of every device-built table (fixed-base multiples here, line coefficients in k_pairk.hip; the host side is
// c12381_hip.hip cached_tables).  A table is HDR_DWORDS of header and its entries; the tables of an array lie tab_stride dwords apart:
//   header[0..47]        the cached point's canonical bytes as dwords (96 B for G1, 192 B for G2)
//   header[HDR_VALID]    1 = table usable (fixed-base: point on the curve, not infinity, in the order-r subgroup; lines: by HDR_RULE)
//   header[HDR_REBUILD]  1 = the build kernel must (re)build, 0 = the cached table matches the point
//   header[HDR_MAGIC]    the header has been written before (a fresh workspace is zeroed: first use is a miss)
//   header[HDR_RULE]     line tables: the rule the table was built under, + 1
// fixed_cache_check_kernel compares and sets HDR_REBUILD, the build kernel that follows it on the stream returns at once on a hit.
// G1 and G2 share the text of the table entry and of the per-lane sums (gate, close, sum, fold): each is ONE body over a group description
// (dev_g1 / dev_g2: fixed_base.hpp's fb_g1 / fb_g2 plus the byte records and the projective records of the finish kernels), and the eight
// kernels of the two groups are one-line calls of their bodies under the names the host, profiles/ and tools/ know.  The two evaluation
// kernels of ONE base are different kernels (the G2 one adds an addend and can write bytes itself) and stay written out.
#include "kernels_common.hpp"
#include "fixed_base.hpp"

using namespace c12381;

namespace c12381 {

// One wavefront per table of the array (blockIdx.x): compare the point with the cached copy; on a miss store the new copy and request a rebuild
__global__ void __launch_bounds__(64, 1) fixed_cache_check_kernel(table_points pts, int nbytes, int32_t* tabs, int tab_stride) {
    int32_t* header = tabs + (size_t)blockIdx.x * tab_stride;
    const int lane = threadIdx.x;
    const int nd = nbytes / 4;
    const uint32_t* b = reinterpret_cast<const uint32_t*>(pts.p[blockIdx.x]);
    uint32_t mine = 0, cached = 0;
    if (lane < nd) { mine = b[lane]; cached = (uint32_t)header[lane]; }
    const bool same = __all(mine == cached) && header[HDR_MAGIC] == 0x46423031;      // magic: the header has been written before
    if (lane < nd) header[lane] = (int32_t)mine;
    if (lane == 0) { header[HDR_REBUILD] = same ? 0 : 1; header[HDR_MAGIC] = 0x46423031; if (!same) header[HDR_VALID] = 0; }
}

// The groups as the bodies below see them.  settle + store: a sum as g*_add leaves it -> the lane's record for the finish kernel (G1 stores
// normalised limbs as they are, g2_store_proj normalises what it is given).  gate = the gate whose HDR_RULE word puts the invalid mark in
// the record's place, or nullptr: no mark; a flag by value makes the G1 mark 42 selects per lane, not one branch (docs/lab_notes.md 12).
struct dev_g1 : fb_g1 {
    static __device__ __forceinline__ void parse(fp& x, fp& y, bool& inf, bool& ok, const uint8_t* src) { g1_parse96(x, y, inf, ok, src); }
    static __device__ __forceinline__ void parse_proj(g1p& p, bool& inf, bool& ok, const uint8_t* src) { g1_parse96_proj(p, inf, ok, src); }
    static __device__ __forceinline__ void one(fp& z) { fp_one(z); }
    static __device__ __forceinline__ void load(g1p& p, const int32_t* proj, size_t stride, size_t i) { soa_load_g1(p, proj, stride, i); }
    static __device__ __forceinline__ void settle(g1p& p) { g1_norm1(p); }
    static __device__ __forceinline__ void store(int32_t* proj, size_t stride, size_t i, g1p& p, const int32_t* gate) {
        if (gate && gate[HDR_RULE] != 0) g1_set_invalid(p);
        soa_store_g1(proj, stride, i, p);
    }
};
struct dev_g2 : fb_g2 {
    static __device__ __forceinline__ void parse(fp2& x, fp2& y, bool& inf, bool& ok, const uint8_t* src) { g2_parse192(x, y, inf, ok, src); }
    static __device__ __forceinline__ void parse_proj(g2p& p, bool& inf, bool& ok, const uint8_t* src) { g2_parse192_proj(p, inf, ok, src); }
    static __device__ __forceinline__ void one(fp2& z) { fp2_one(z); }
    static __device__ __forceinline__ void load(g2p& p, const int32_t* proj, size_t stride, size_t i) { soa_load_g2(p, proj, stride, i); }
    static __device__ __forceinline__ void settle(g2p&) {}
    static __device__ __forceinline__ void store(int32_t* proj, size_t stride, size_t i, g2p& p, const int32_t* gate) {
        g2_store_proj(proj, stride, i, p, gate && gate[HDR_RULE] != 0);
    }
};

// The tables of a set of bases (POINT_BYTES apart) in one launch: blockIdx.y = base, every entry by its own lane (no entry waits for
// another); a base whose cached table is current costs its workgroups one load.  A single table is an array of one.
template <class G>
static __device__ __forceinline__ void fixed_tables_body(const uint8_t* bases, int32_t* tabs, int tab_stride) {
    const uint8_t* src = bases + (size_t)G::POINT_BYTES * blockIdx.y;
    int32_t* header = tabs + (size_t)blockIdx.y * tab_stride;
    const size_t L = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (header[HDR_REBUILD] == 0) return;                                   // cached table is current
    if (L >= (size_t)G::WINDOWS * FB_ENTRIES) return;
    typename G::point base;
    bool inf, ok;
    G::parse(base.x, base.y, inf, ok, src);
    G::one(base.z);
    if (L == 0) header[HDR_VALID] = (ok && !inf && G::in_subgroup(base)) ? 1 : 0;
    if (!ok || inf) return;
    fixed_table_put<G>(header + FB_HEADER_DWORDS + L * G::ENTRY_DWORDS, base, L);
}
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_tables_kernel(const uint8_t* bases96, int32_t* tabs, int tab_stride) {
    fixed_tables_body<dev_g1>(bases96, tabs, tab_stride);
}
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_tables_kernel(const uint8_t* bases192, int32_t* tabs, int tab_stride) {
    fixed_tables_body<dev_g2>(bases192, tabs, tab_stride);
}

// proj[off + i] = [k_i]B from the table; does nothing when the table is not valid (the generic kernel runs then)
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_eval_kernel(size_t n, const int32_t* buf, const uint8_t* scalars, int32_t* proj, size_t proj_stride,
                                                              size_t proj_off) {
    if (buf[HDR_VALID] == 0) return;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t raw[8], k[8];
    load_raw32(raw, scalars + 32 * i);
    scalar_from_raw32(k, raw);
    g1p acc, o;
    g1_fixed_eval(acc, buf + FB_HEADER_DWORDS, k);
    g1_norm1(o, acc);
    soa_store_g1(proj, proj_stride, proj_off + i, o);
}

// out[i] = addend + [k_i]Q (affine, canonical 192 B or 97 B — or projective SoA for g2_finish_kernel when proj is given);
// addend = one broadcast 192-byte point or nullptr.  Does nothing when the table is not valid.
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_eval_kernel(size_t n, const int32_t* buf, const uint8_t* scalars, const uint8_t* addend192,
                                                              uint8_t* out, int fmt, int* bad_flag, int32_t* proj, size_t proj_stride) {
    if (buf[HDR_VALID] == 0) return;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t raw[8], k[8];
    load_raw32(raw, scalars + 32 * i);
    scalar_from_raw32(k, raw);
    g2p acc;
    g2_fixed_eval(acc, buf + FB_HEADER_DWORDS, k);
    bool wok = true;
    if (addend192) {                                      // kernel-uniform
        g2p w;
        bool winf;
        g2_parse192_proj(w, winf, wok, addend192);
        if (!wok) *bad_flag = 1;
        g2_norm1(acc, acc);
        g2_add(acc, w);
    }
    if (proj) g2_store_proj(proj, proj_stride, i, acc, !wok);                // kernel-uniform: affine conversion by g2_finish_kernel
    else g2_store_affine(out + (size_t)fmt * i, acc, fmt, !wok);
}


// ---- per-lane sums over a set of shared bases (c12381_g{1,2}_mul_fixed_sum_batch): out[j] = addend + sum_i [k_(i n + j)]B_i
// The gate in front of the nb tables picks the route on the device: gate[HDR_VALID] = every base has a valid table (the sum kernel
// runs), (gate + GATE_OTHER)[HDR_VALID] = the opposite (the generic columns and the fold kernel run), gate[HDR_RULE] = a base or
// the addend is not on the curve / twist (every output is marked invalid; *bad_flag is raised here, once).  One wavefront: lane t looks at
// base t, lane nb at the addend.
template <class G>
static __device__ __forceinline__ void fixed_sum_gate_body(int nb, const uint8_t* bases, const uint8_t* addend, int32_t* gate, const int32_t* tabs,
                                                           int tab_stride, int use_tables, int* bad_flag) {
    const int t = threadIdx.x;
    bool ok = true, valid = true;
    if (t < nb || (t == nb && addend)) {
        typename G::coord x, y;
        bool inf;
        G::parse(x, y, inf, ok, t < nb ? bases + G::POINT_BYTES * t : addend);
    }
    if (t < nb) valid = use_tables && tabs[(size_t)t * tab_stride + HDR_VALID] != 0;
    const bool all_valid = __all(valid), bad = __any(!ok);
    if (t == 0) {
        gate[HDR_VALID] = all_valid ? 1 : 0;
        gate[GATE_OTHER + HDR_VALID] = all_valid ? 0 : 1;
        gate[HDR_RULE] = bad ? 1 : 0;
        if (bad) *bad_flag = 1;
    }
}
// acc -> the lane's record for the finish kernel: plus the addend (complete addition, as g1_add_const_kernel and g2_fixed_eval_kernel add
// it), or the invalid mark when the gate says so
template <class G>
static __device__ __forceinline__ void fixed_sum_close(int32_t* proj, size_t proj_stride, size_t j, const typename G::point& acc, const uint8_t* addend,
                                                       const int32_t* gate) {
    typename G::point o;
    G::norm1(o, acc);
    if (addend) {                                         // kernel-uniform
        typename G::point q;
        bool inf, ok;
        G::parse_proj(q, inf, ok, addend);
        G::add(o, q);
        G::settle(o);
    }
    G::store(proj, proj_stride, j, o, gate);
}
// lane j's 32-byte scalar for base i of a base-major array of nb x n records
struct fixed_sum_scalars {
    const uint8_t* sc; size_t n, j;
    __device__ __forceinline__ void operator()(int i, uint32_t (&k)[8]) const {
        uint32_t raw[8];
        load_raw32(raw, sc + 32 * ((size_t)i * n + j));
        scalar_from_raw32(k, raw);
    }
};
// proj[j] = addend + sum_(i < nb) [k_(i n + j)]B_i from the nb tables behind the gate: one lane per output, one accumulator per lane in
// registers across all bases, no per-column store and no reduce pass
template <class G>
static __device__ __forceinline__ void fixed_sum_body(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride, const uint8_t* scalars,
                                                      const uint8_t* addend, int32_t* proj, size_t proj_stride) {
    if (gate[HDR_VALID] == 0) return;
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    typename G::point acc;
    fixed_eval_sum<G>(acc, tabs + FB_HEADER_DWORDS, (size_t)tab_stride, nb, fixed_sum_scalars{scalars, n, j});
    fixed_sum_close<G>(proj, proj_stride, j, acc, addend, gate);
}
// The generic route, column by column: proj[j] += proj[col_off + j] (has_col), and behind the last column the addend / invalid mark (last)
template <class G>
static __device__ __forceinline__ void fixed_sum_fold_body(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off, int has_col,
                                                           int last, const uint8_t* addend) {
    if (gate[GATE_OTHER + HDR_VALID] == 0) return;
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    typename G::point acc;
    G::load(acc, proj, proj_stride, j);
    if (has_col) {
        typename G::point q;
        G::load(q, proj, proj_stride, col_off + j);
        G::add(acc, q);
    }
    if (last) fixed_sum_close<G>(proj, proj_stride, j, acc, addend, gate);
    else { G::settle(acc); G::store(proj, proj_stride, j, acc, nullptr); }
}
__global__ void __launch_bounds__(64, 1) g1_fixed_sum_gate_kernel(int nb, const uint8_t* bases96, const uint8_t* addend96, int32_t* gate,
                                                                 const int32_t* tabs, int tab_stride, int use_tables, int* bad_flag) {
    fixed_sum_gate_body<dev_g1>(nb, bases96, addend96, gate, tabs, tab_stride, use_tables, bad_flag);
}
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_sum_kernel(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride,
                                                             const uint8_t* scalars, const uint8_t* addend96, int32_t* proj, size_t proj_stride) {
    fixed_sum_body<dev_g1>(n, nb, gate, tabs, tab_stride, scalars, addend96, proj, proj_stride);
}
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_sum_fold_kernel(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off,
                                                                  int has_col, int last, const uint8_t* addend96) {
    fixed_sum_fold_body<dev_g1>(n, gate, proj, proj_stride, col_off, has_col, last, addend96);
}
__global__ void __launch_bounds__(64, 1) g2_fixed_sum_gate_kernel(int nb, const uint8_t* bases192, const uint8_t* addend192, int32_t* gate,
                                                                 const int32_t* tabs, int tab_stride, int use_tables, int* bad_flag) {
    fixed_sum_gate_body<dev_g2>(nb, bases192, addend192, gate, tabs, tab_stride, use_tables, bad_flag);
}
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_sum_kernel(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride,
                                                             const uint8_t* scalars, const uint8_t* addend192, int32_t* proj, size_t proj_stride) {
    fixed_sum_body<dev_g2>(n, nb, gate, tabs, tab_stride, scalars, addend192, proj, proj_stride);
}
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_sum_fold_kernel(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off,
                                                                  int has_col, int last, const uint8_t* addend192) {
    fixed_sum_fold_body<dev_g2>(n, gate, proj, proj_stride, col_off, has_col, last, addend192);
}

}  // namespace c12381
