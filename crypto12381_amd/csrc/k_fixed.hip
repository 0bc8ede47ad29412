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

// entry L of the table of base96 (every entry by its own lane: no entry waits for another)
static __device__ __forceinline__ void g1_fixed_table_entry(const uint8_t* base96, int32_t* buf, size_t L) {
    int32_t* header = buf;
    if (header[HDR_REBUILD] == 0) return;                                   // cached table is current
    if (L >= (size_t)FB_G1_WINDOWS * FB_ENTRIES) return;
    g1p base;
    bool inf, ok;
    g1_parse96(base.x, base.y, inf, ok, base96);
    fp_one(base.z);
    if (L == 0) header[HDR_VALID] = (ok && !inf && g1_in_subgroup(base)) ? 1 : 0;
    if (!ok || inf) return;
    const int j = (int)(L / FB_ENTRIES);
    const uint32_t d = (uint32_t)(L % FB_ENTRIES) + 1u;
    g1p acc;
    g1_fixed_entry(acc, base, d, 8 * j);
    fp zn, zi, ax, ay;
    fp_norm1(zn, acc.z);
    fp_inv(zi, zn);
    g1p an;
    g1_norm1(an, acc);
    g1_to_affine(ax, ay, an, zi);
    msm_store_pt(buf + FB_HEADER_DWORDS + L * FB_G1_DWORDS, ax, ay);
}
// the tables of a set of bases (96 bytes apart) in one launch: blockIdx.y = base; a base whose cached table is current costs its workgroups one load
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_tables_kernel(const uint8_t* bases96, int32_t* tabs, int tab_stride) {
    g1_fixed_table_entry(bases96 + (size_t)96 * blockIdx.y, tabs + (size_t)blockIdx.y * tab_stride, (size_t)blockIdx.x * BLOCK + threadIdx.x);
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

// ---- per-lane sums over a set of shared bases (c12381_g1_mul_fixed_sum_batch): out[j] = addend + sum_i [k_(i n + j)]B_i
// The gate in front of the nb tables picks the route on the device: gate[HDR_VALID] = every base has a valid table (g1_fixed_sum_kernel
// runs), (gate + GATE_OTHER)[HDR_VALID] = the opposite (the generic columns and g1_fixed_sum_fold_kernel run), gate[HDR_RULE] = a base or
// the addend is not on the curve (every output is marked invalid; *bad_flag is raised here, once).  One wavefront: lane t looks at base t,
// lane nb at the addend.
__global__ void __launch_bounds__(64, 1) g1_fixed_sum_gate_kernel(int nb, const uint8_t* bases96, const uint8_t* addend96, int32_t* gate,
                                                                 const int32_t* tabs, int tab_stride, int use_tables, int* bad_flag) {
    const int t = threadIdx.x;
    bool ok = true, valid = true;
    if (t < nb || (t == nb && addend96)) {
        fp x, y;
        bool inf;
        g1_parse96(x, y, inf, ok, t < nb ? bases96 + 96 * t : addend96);
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
// acc -> the lane's result: plus the addend (complete addition, as g1_add_const_kernel), or the invalid mark when the gate says so
static __device__ __forceinline__ void g1_fixed_sum_close(g1p& o, const g1p& acc, const uint8_t* addend96, const int32_t* gate) {
    g1_norm1(o, acc);
    if (addend96) {                                       // kernel-uniform
        g1p q;
        bool inf, ok;
        g1_parse96_proj(q, inf, ok, addend96);
        g1_add(o, q);
        g1_norm1(o);
    }
    if (gate[HDR_RULE] != 0) g1_set_invalid(o);
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
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_sum_kernel(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride,
                                                             const uint8_t* scalars, const uint8_t* addend96, int32_t* proj, size_t proj_stride) {
    if (gate[HDR_VALID] == 0) return;
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g1p acc, o;
    g1_fixed_eval_sum(acc, tabs + FB_HEADER_DWORDS, (size_t)tab_stride, nb, fixed_sum_scalars{scalars, n, j});
    g1_fixed_sum_close(o, acc, addend96, gate);
    soa_store_g1(proj, proj_stride, j, o);
}
// The generic route, column by column: proj[j] += proj[col_off + j] (has_col), and behind the last column the addend / invalid mark (last)
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_sum_fold_kernel(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off,
                                                                  int has_col, int last, const uint8_t* addend96) {
    if (gate[GATE_OTHER + HDR_VALID] == 0) return;
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g1p acc, o;
    soa_load_g1(acc, proj, proj_stride, j);
    if (has_col) {
        g1p q;
        soa_load_g1(q, proj, proj_stride, col_off + j);
        g1_add(acc, q);
    }
    if (last) g1_fixed_sum_close(o, acc, addend96, gate);
    else g1_norm1(o, acc);
    soa_store_g1(proj, proj_stride, j, o);
}

// entry L of the table of base192, as g1_fixed_table_entry
static __device__ __forceinline__ void g2_fixed_table_entry(const uint8_t* base192, int32_t* buf, size_t L) {
    int32_t* header = buf;
    if (header[HDR_REBUILD] == 0) return;                                   // cached table is current
    if (L >= (size_t)FB_G2_WINDOWS * FB_ENTRIES) return;
    g2p base;
    bool inf, ok;
    g2_parse192(base.x, base.y, inf, ok, base192);
    fp2_one(base.z);
    if (L == 0) header[HDR_VALID] = (ok && !inf && g2_in_subgroup(base)) ? 1 : 0;
    if (!ok || inf) return;
    const int j = (int)(L / FB_ENTRIES);
    const uint32_t d = (uint32_t)(L % FB_ENTRIES) + 1u;
    g2p acc;
    g2_fixed_entry(acc, base, d, 8 * j);
    fp2 zn, zi, ax, ay;
    fp2_norm1(zn, acc.z);
    fp2_inv(zi, zn);
    fp2_mul(ax, acc.x, zi); fp2_mul(ay, acc.y, zi);
    fp2_norm1(ax, ax); fp2_norm1(ay, ay);
    fb_store_g2(buf + FB_HEADER_DWORDS + L * FB_G2_DWORDS, ax, ay);
}
// the tables of a set of bases (192 bytes apart) in one launch: blockIdx.y = base, as g1_fixed_tables_kernel; the single table of
// c12381_g2_mul_fixed_batch is an array of one
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_tables_kernel(const uint8_t* bases192, int32_t* tabs, int tab_stride) {
    g2_fixed_table_entry(bases192 + (size_t)192 * blockIdx.y, tabs + (size_t)blockIdx.y * tab_stride, (size_t)blockIdx.x * BLOCK + threadIdx.x);
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
        g2p w, inf_pt;
        bool winf;
        g2_parse192(w.x, w.y, winf, wok, addend192);
        fp2_one(w.z);
        g2_set_inf(inf_pt);
        fp2_select(w.x, winf, inf_pt.x, w.x); fp2_select(w.y, winf, inf_pt.y, w.y); fp2_select(w.z, winf, inf_pt.z, w.z);
        if (!wok) *bad_flag = 1;
        g2_norm1(acc, acc);
        g2_add(acc, w);
    }
    if (proj) g2_store_proj(proj, proj_stride, i, acc, !wok);                // kernel-uniform: affine conversion by g2_finish_kernel
    else g2_store_affine(out + (size_t)fmt * i, acc, fmt, !wok);
}

// ---- per-lane sums over a set of shared G2 bases (c12381_g2_mul_fixed_sum_batch): out[j] = addend + sum_i [k_(i n + j)]Q_i
// The gate words and the two routes are those of the G1 form above (g1_fixed_sum_gate_kernel): gate[HDR_VALID] = every base has a valid
// table, (gate + GATE_OTHER)[HDR_VALID] = the opposite, gate[HDR_RULE] = a base or the addend is not on the twist.
__global__ void __launch_bounds__(64, 1) g2_fixed_sum_gate_kernel(int nb, const uint8_t* bases192, const uint8_t* addend192, int32_t* gate,
                                                                 const int32_t* tabs, int tab_stride, int use_tables, int* bad_flag) {
    const int t = threadIdx.x;
    bool ok = true, valid = true;
    if (t < nb || (t == nb && addend192)) {
        fp2 x, y;
        bool inf;
        g2_parse192(x, y, inf, ok, t < nb ? bases192 + 192 * t : addend192);
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
// acc -> the lane's record for g2_finish_kernel: plus the addend (complete addition, as g2_fixed_eval_kernel adds it), or the invalid mark
// when the gate says so
static __device__ __forceinline__ void g2_fixed_sum_close(int32_t* proj, size_t proj_stride, size_t j, const g2p& acc, const uint8_t* addend192,
                                                          const int32_t* gate) {
    g2p o;
    g2_norm1(o, acc);
    if (addend192) {                                      // kernel-uniform
        g2p w, inf_pt;
        bool winf, wok;
        g2_parse192(w.x, w.y, winf, wok, addend192);
        fp2_one(w.z);
        g2_set_inf(inf_pt);
        fp2_select(w.x, winf, inf_pt.x, w.x); fp2_select(w.y, winf, inf_pt.y, w.y); fp2_select(w.z, winf, inf_pt.z, w.z);
        g2_add(o, w);
    }
    g2_store_proj(proj, proj_stride, j, o, gate[HDR_RULE] != 0);
}
// proj[j] = addend + sum_(i < nb) [k_(i n + j)]Q_i from the nb tables behind the gate: one lane per output, one accumulator per lane
// across all bases, no per-column store and no reduce pass
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_sum_kernel(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride,
                                                             const uint8_t* scalars, const uint8_t* addend192, int32_t* proj, size_t proj_stride) {
    if (gate[HDR_VALID] == 0) return;
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g2p acc;
    g2_fixed_eval_sum(acc, tabs + FB_HEADER_DWORDS, (size_t)tab_stride, nb, fixed_sum_scalars{scalars, n, j});
    g2_fixed_sum_close(proj, proj_stride, j, acc, addend192, gate);
}
// The generic route, column by column: proj[j] += proj[col_off + j] (has_col), and behind the last column the addend / invalid mark (last)
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_sum_fold_kernel(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off,
                                                                  int has_col, int last, const uint8_t* addend192) {
    if (gate[GATE_OTHER + HDR_VALID] == 0) return;
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g2p acc;
    soa_load_g2(acc, proj, proj_stride, j);
    if (has_col) {
        g2p q;
        soa_load_g2(q, proj, proj_stride, col_off + j);
        g2_add(acc, q);
    }
    if (last) g2_fixed_sum_close(proj, proj_stride, j, acc, addend192, gate);
    else g2_store_proj(proj, proj_stride, j, acc, false);
}


}  // namespace c12381
