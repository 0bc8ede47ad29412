// Kernel entry points of the backend, one translation unit per family so the families compile in parallel:
//   k_g1.hip     Fp hooks, G1 scalar multiplication / addition / finish / tree sum, MSM stages, G1 decompression
//   k_g1sum.hip  per-lane sums of K G1 products under one doubling chain (K co-Z tables on one common Z)
//   k_g2gt.hip   G2 scalar multiplication (one lane per point) / addition / finish / decompression, one-lane pairing kernels, GT arithmetic
//   k_g2h.hip    G2 scalar multiplication with two lanes per point (half an Fp2 element per lane)
//   k_pair3.hip  three-lanes-per-pairing Miller loop + final exponentiation
//   k_hash_zp.hip  hash-to-G1 and the scalar-field (Zp) helpers
//   k_pairk.hip  K-way pairing products against fixed G2 points (line tables, prep, work-queue kernels)
//   k_fixed.hip  fixed-base tables and their evaluation (public-parameter columns of BBS+)
//   k_bbs04.hip  SHA3-512 (sha3.hpp) and the bbs04 group-signature stages around the scalar multiplications and the pairing product
//   k_ps.hip     the PS signature stages (ps.hpp) around decompression, the fixed-base column, the bucket products and the pairing product
//   k_ac_bbs.hip the AC-bbs credential stages (ac_bbs.hpp) around decompression, the fixed-base sums, the k-way products and PS verification
//   k_ac_rbbs.hip the AC-rbbs credential stages (ac_rbbs.hpp): the same, with the q_i hashes, the exponents of redact and a second pairing equation
//   k_ac_rps.hip the AC-rps credential stages (ac_rps.hpp): the q_k hashes over points and indices, the exponents of pres, G2 subtraction
//   k_mhac_bbs.hip the MHAC-bbs credential stages (mhac_bbs.hpp): the index sets, the transcript over revealed values, the threshold responses
//   k_mhac_iss.hip the MHAC-bbs issuance stages (mhac_iss.hpp): the polynomial shares, the Lagrange columns, the row gather, the records and statuses
//   k_ac_issue.hip the AC issuance stages (ac_issue.hpp): the issuer's scalars — x + w; the Horner sum and the power of y —, the records and statuses
// c12381_hip.hip (context, workspaces, C ABI) launches them.  Every kernel is built for 2 waves per SIMD
// (__launch_bounds__(BLOCK, 2)): the field routines are not inlined and get the full 256-VGPR budget.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace c12381 {

constexpr int BLOCK = 256;
constexpr int FINISH_M = 16;                     // most elements per lane in the simultaneous inversion (c12381_hip.hip finish_lanes)
constexpr int TRI_PER_WAVE = 21;                 // pairings per 64-lane wavefront in the three-lane kernels (lane 63 idles along)
// Header words in front of a device-built table (fixed-base multiples, line coefficients) and of a gate buffer; the protocol: k_fixed.hip
constexpr int HDR_VALID = 48;                    // 1 = table usable / this path runs; kernels of the other path return at once
constexpr int HDR_REBUILD = 49;                  // set by fixed_cache_check_kernel (the one check kernel of every table array) when the cached point differs
constexpr int HDR_MAGIC = 50;                    // the header has been written before
constexpr int HDR_RULE = 51;                     // validity rule the flag was computed under (line tables)
constexpr int HDR_DWORDS = 64;                   // table data starts here
int set_queue_groups_override(int v);             // k_pair3.hip: tuning switch (C12381_QUEUE_GROUPS), read by gt3_pow_queue_kernel alone
constexpr int GATE_OTHER = 49;                   // (gate + GATE_OTHER)[HDR_VALID] = the complement of gate[HDR_VALID]

// Waves per SIMD of the three scalar-multiplication kernels (register budget 512 / occupancy: 256, 168 or 128 VGPRs).  Three per SIMD were
// measured twice and lose: the spills cost more than the third wavefront fills (profiles/r03_ab_occupancy.txt, r04_ab_occupancy3.txt).
constexpr int G1_OCC = 2, MSM_OCC = 2, G2H_OCC = 2;
__global__ void __launch_bounds__(BLOCK, 2) fp_op_kernel(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) fp_mulchain_kernel(size_t n, int iters, const uint8_t* a, const uint8_t* b, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_kernel(size_t n, const uint8_t* pts, size_t pt_stride, const uint8_t* scalars, int32_t* tab, int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, const int32_t* skip_if, int small_term);
// k_g1sum.hip: out[i] = sum_(j < K) [k_(j col + i)]P_(j col + i), K = 2, 3, 4 terms per lane (one term is g1_mul_kernel); tab holds K records per lane
constexpr int G1_MUL_SUM_MAX = 4;
__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_sum2_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab, int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, int small_term);
__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_sum3_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab, int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, int small_term);
__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_sum4_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab, int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, int small_term);
__global__ void __launch_bounds__(BLOCK, 2) g1_rsub_kernel(size_t n, int32_t* acc, size_t acc_stride, const int32_t* other, size_t other_stride, size_t other_off, const int32_t* run_if);
__global__ void __launch_bounds__(BLOCK, 2) g1_add_kernel(size_t n, const uint8_t* a, const uint8_t* b, int32_t* proj, size_t proj_stride, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) g1_finish_kernel(size_t n, const int32_t* proj, size_t stride, int32_t* pref, uint8_t* out, int fmt, size_t T);
__global__ void __launch_bounds__(BLOCK, 2) g1_lift_kernel(size_t n, const uint8_t* pts, int32_t* proj, size_t stride, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) g1_reduce_kernel(size_t n, const int32_t* in, size_t in_stride, size_t m, int32_t* outp, size_t out_stride);
__global__ void __launch_bounds__(BLOCK, 2) g1_mul_plain_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, int32_t* proj, size_t proj_stride, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) g1_add_const_kernel(size_t n, int32_t* proj, size_t stride, const uint8_t* pt96, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) msm_prep_kernel(size_t n, const uint8_t* pts, int in_fmt, const uint8_t* scalars, int c, int W, int32_t* pts2, uint32_t* keys, uint32_t* vals, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) msm_ranges_kernel(size_t E, const uint32_t* keys, int c, int W, uint32_t* lo, uint32_t* hi);
__global__ void __launch_bounds__(BLOCK, 2) msm_prep16_kernel(size_t n, const uint8_t* pts, int in_fmt, const uint8_t* scalars, int c, int W, int32_t* pts2, uint16_t* keys, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) msm_ranges16_kernel(size_t n, const uint16_t* keys, int c, int W, uint32_t* lo, uint32_t* hi);
constexpr int MSM_RANGES_PER_THREAD = 8;           // entries per thread of msm_ranges16_kernel (the host sizes its grid with it)
__global__ void __launch_bounds__(BLOCK, MSM_OCC) msm_bucket_kernel(size_t nbk, const uint32_t* lo, const uint32_t* hi, const uint32_t* vals, const int32_t* pts2, int32_t* bk, const uint32_t* order, uint32_t cap, uint32_t early_max);
__global__ void __launch_bounds__(BLOCK, 2) msm_sizes_kernel(size_t nbk, const uint32_t* lo, const uint32_t* hi, uint32_t* key, uint32_t* ident, uint32_t cap, uint32_t* cnt, uint2* seg, uint4* big, uint32_t early_max);
__global__ void __launch_bounds__(BLOCK, 2) msm_overflow_kernel(const uint32_t* cnt, const uint2* seg, const uint32_t* lo, const uint32_t* hi, const uint32_t* vals, const int32_t* pts2, int32_t* part, uint32_t cap);
__global__ void __launch_bounds__(BLOCK, 2) msm_overflow_combine_kernel(const uint32_t* cnt, const uint4* big, const int32_t* part, int32_t* bk);
__global__ void __launch_bounds__(BLOCK, 2) msm_wreduce_kernel(int W, uint32_t nb, uint32_t chunks, const int32_t* bk, int32_t* out, size_t out_stride);
__global__ void __launch_bounds__(BLOCK, 2) g1_decompress_kernel(size_t n, const uint8_t* in, uint8_t* out, uint8_t* status, int mark_invalid);
__global__ void __launch_bounds__(64, 1) msm_horner_kernel(const int32_t* rw, size_t stride, int W, int c, int32_t* out, size_t out_stride, const int32_t* term_in);
__global__ void __launch_bounds__(BLOCK, 2) g1_wave_reduce_kernel(size_t groups, int W, const int32_t* in, size_t in_stride, int32_t* outp, size_t out_stride);
__global__ void __launch_bounds__(64, 1) msm_small_term_kernel(const int32_t* sbucket, int32_t* term_out, const uint32_t* done);
__global__ void __launch_bounds__(64, 1) msm_small_early_kernel(const uint32_t* lo, const uint32_t* hi, uint32_t small_bucket, uint32_t early_max, const uint32_t* vals, const int32_t* pts2, int32_t* term_out, uint32_t* done);
constexpr uint32_t MSM_SMALL_EARLY_MAX = 4096;     // longest small-scalar bucket msm_small_early_kernel takes (64 additions per lane)
__global__ void __launch_bounds__(BLOCK, 2) g2_mul_kernel(size_t n, const uint8_t* pts, size_t pt_stride, const uint8_t* scalars, int32_t* tab, size_t tab_stride, uint8_t* out, int fmt, int* bad_flag, const int32_t* skip_if, int32_t* proj, size_t proj_stride, size_t proj_off, int in_g2);
__global__ void __launch_bounds__(BLOCK, G2H_OCC) g2_mul2_kernel(size_t n, const uint8_t* pts, size_t pt_stride, const uint8_t* scalars, int32_t* tab, int* bad_flag, const int32_t* skip_if, int32_t* proj, size_t proj_stride, size_t proj_off, int in_g2);
__global__ void __launch_bounds__(BLOCK, 2) g2_finish_kernel(size_t n, const int32_t* proj, size_t stride, int32_t* pref, uint8_t* out, int fmt, size_t T);
__global__ void __launch_bounds__(BLOCK, 2) g2_lift_kernel(size_t n, const uint8_t* pts, int32_t* proj, size_t stride, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) g2_reduce_kernel(size_t n, const int32_t* in, size_t in_stride, size_t m, int32_t* outp, size_t out_stride);
__global__ void __launch_bounds__(BLOCK, 2) g2_add_kernel(size_t n, const uint8_t* a, size_t a_stride, const uint8_t* b, uint8_t* out, int fmt, int* bad_flag, const int32_t* skip_if);
#ifdef C12381_EXPERIMENTS      // the superseded one-lane pairing kernels (k_g2gt.hip): experiments builds only
__global__ void __launch_bounds__(BLOCK, 2) clock_probe_kernel(unsigned long long* out, int n, int gap);
__global__ void __launch_bounds__(BLOCK, 2) pair_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) pair_eq_kernel(size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, size_t b2_stride, uint8_t* out, int* bad_flag);
#endif
__global__ void __launch_bounds__(BLOCK, 2) g2_decompress_kernel(size_t n, const uint8_t* in, uint8_t* out, uint8_t* status, int mark_invalid);
#ifdef C12381_EXPERIMENTS
__global__ void __launch_bounds__(BLOCK, 2) miller_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) gt_op_kernel(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) gt_is_unity_kernel(size_t n, const uint8_t* a, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) fp_raw_kernel(int op, size_t n, const int32_t* in, const int32_t* kk, int32_t* out);   // k_fp_raw.hip: raw-limb test kernel
__global__ void __launch_bounds__(BLOCK, 2) fp2h_raw_kernel(int op, size_t n, const int32_t* in, const int32_t* kk, int32_t* out);  // the same, two lanes per element (fp2h.hpp)
#endif
__global__ void __launch_bounds__(BLOCK, 2) pair3_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) pair3_prod_kernel(size_t n, int k, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag, int miller_only);
__global__ void __launch_bounds__(BLOCK, 2) pair3_eq_kernel(size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, size_t b2_stride, uint8_t* out, int* bad_flag, const int32_t* skip_if);
__global__ void __launch_bounds__(BLOCK, 2) miller3_queue_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch, unsigned long long* wstats);
__global__ void __launch_bounds__(BLOCK, 2) fexp3_queue_kernel(size_t n, const uint8_t* in576, uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch, unsigned long long* wstats);
__global__ void __launch_bounds__(BLOCK, 2) pair3_queue_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch, unsigned long long* stamps, unsigned long long* wstats);
__global__ void __launch_bounds__(BLOCK, 2) pair3_eq_queue_kernel(size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, size_t b2_stride, uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, const int32_t* skip_if, size_t ndirect, int spin_limit, unsigned int epoch);
__global__ void __launch_bounds__(BLOCK, 2) pair3_prod_fixed_queue_kernel(size_t n, const uint8_t* a96, const uint8_t* c96, const int32_t* tabw, const int32_t* tabg, uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, const int32_t* run_if, size_t ndirect, int spin_limit, unsigned int epoch);
__global__ void __launch_bounds__(BLOCK, 2) pair3_fixed_queue_kernel(size_t n, const uint8_t* g1_96, const int32_t* buf, uint8_t* gt, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch);
// k_pairk.hip: K-way products of pairings against fixed G2 points (C12381_FIXED_G2_MAX = FIXED_G2_MAX); the point columns travel by value
constexpr int FIXED_G2_MAX = 8;
struct g1_cols { const uint8_t* p[FIXED_G2_MAX]; };
struct g2_cols { const uint8_t* p[FIXED_G2_MAX]; };
__global__ void __launch_bounds__(BLOCK, 2) g2_lines_tables_kernel(int k, g2_cols q, int32_t* tabs, int tab_stride, int rule);   // rule: bit 0 need_g2, bit 1 raw records
__global__ void __launch_bounds__(BLOCK, 2) gate_all_kernel(int32_t* gate, const int32_t* tabs, int tab_stride, int k);
__global__ void __launch_bounds__(BLOCK, 2) pairk_prep_kernel(size_t n, int k, g1_cols cols, uint32_t neg_mask, int32_t* pts, uint32_t* mask, const int32_t* skip_if);
__global__ void __launch_bounds__(BLOCK, 2) g2_bcast_kernel(size_t n, const uint8_t* src, uint8_t* dst, const int32_t* skip_if);
__global__ void __launch_bounds__(BLOCK, 2) pair3_prodk_fixed_queue_kernel(size_t n, int k, const int32_t* pts, const uint32_t* mask, const int32_t* tabs, int tab_stride, uint8_t* gt, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, const int32_t* gate, size_t ndirect, int miller_only, int spin_limit, unsigned int epoch);
__global__ void __launch_bounds__(BLOCK, 2) pair3_prodk_fixed_eq_queue_kernel(size_t n, int k, const int32_t* pts, const uint32_t* mask, const int32_t* tabs, int tab_stride, uint8_t* ok, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, const int32_t* run_if, size_t ndirect, int spin_limit, unsigned int epoch);
__global__ void __launch_bounds__(BLOCK, 2) miller3_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) gt3_op_kernel(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, uint4* pow_tab);
__global__ void __launch_bounds__(BLOCK, 2) gt3_pow_queue_kernel(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, int* bad_flag, uint4* pow_tab, uint4* state, unsigned int* flags, unsigned int* counter, int spin_limit);
constexpr size_t GT_POW_TAB_BYTES_PER_WAVE = (size_t)16 * 14 * 64 * 16;   // 16 entries x 14 rows (one Fp4 per lane) x 64 lanes x 16 bytes
__global__ void __launch_bounds__(BLOCK, 2) gt3_is_unity_kernel(size_t n, const uint8_t* a, uint8_t* out);
constexpr int PAIR_QUEUE_STATE_ROWS = 42;        // 16-byte rows x 64 lanes per group of 21 pairings (F, tc1, tc2, y1): the fenced form (GT power queue)
constexpr size_t PAIR_QUEUE_STATE_BYTES = (size_t)168 * 64 * 8;   // a queued group's block: 168 32-bit words per lane, each in an 8-byte tagged word (pair_queue.hpp stw_store)
__global__ void __launch_bounds__(BLOCK, 2) g1_from_hash_kernel(size_t n, const uint8_t* in, int mode, int32_t* proj, size_t proj_stride, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) zp_op_kernel(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) zp_fold_cols_kernel(size_t n, const uint8_t* a, size_t a_col_stride, const uint8_t* r32, const uint8_t* m32, int first, size_t T, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) bbs_wire_pub_kernel(size_t nblk, const uint8_t* g1_g2_h0, const uint8_t* h49, const uint8_t* pk97, uint8_t* g1s49, uint8_t* g2s97);
__global__ void __launch_bounds__(BLOCK, 2) bbs_wire_prep_kernel(size_t n, size_t msg_len, size_t nblk, const uint8_t* sig145, const uint8_t* msgs, uint8_t* a49, uint8_t* x32, uint8_t* r32, uint8_t* m32, uint8_t* status);
__global__ void __launch_bounds__(BLOCK, 2) bbs_wire_finish_kernel(size_t n, size_t npub1, const uint8_t* st_sig, const uint8_t* st_a, const uint8_t* st_pub1, const uint8_t* st_pub2, uint8_t* ok, int* bad_flag);
constexpr int ZP_INV_RUN = 16;
__global__ void __launch_bounds__(BLOCK, 2) zp_batch_inv_kernel(size_t n, size_t T, const uint8_t* x, const uint8_t* gamma, uint8_t* out, uint32_t* pref);
__global__ void __launch_bounds__(BLOCK, 2) zp_from_hash_kernel(size_t n, const uint8_t* digests, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) zp_fold_kernel(size_t n, const uint8_t* a, const uint8_t* b, size_t T, uint8_t* out);
// k_bbs04.hip: SHA3-512 and the bbs04 group-signature kernels
__global__ void __launch_bounds__(BLOCK, 2) sha3_512_kernel(size_t n, size_t len, const uint8_t* msgs, uint8_t* out64);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_pub_kernel(const uint8_t* gpk390, uint8_t* g1s49, uint8_t* g2s97);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_prep_kernel(size_t n, const uint8_t* sig435, uint8_t* t49, uint8_t* sc, uint8_t* c32, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_combine_kernel(size_t n, int32_t* proj, size_t stride);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_transcript_kernel(size_t n, size_t msg_len, const uint8_t* msgs, const uint8_t* t49, const uint8_t* t96, const uint8_t* r49, const uint8_t* gt576, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_check_kernel(size_t n, size_t L, const uint8_t* tr, const uint8_t* c32, const uint8_t* st_sig, const uint8_t* st_t, const uint8_t* st_pub, uint8_t* ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_open_prep_kernel(size_t n, const uint8_t* gmsk96, const uint8_t* sig435, uint8_t* t49, uint8_t* sc, uint8_t* st, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_open_combine_kernel(size_t n, int32_t* proj, size_t stride, const uint8_t* t3_96);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_open_status_kernel(size_t n, const uint8_t* st_sig, const uint8_t* st_t, uint8_t* status);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_prep_kernel(size_t n, const uint8_t* gsk97, const uint8_t* rnd224, uint8_t* a49, uint8_t* sc);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_t3_kernel(size_t n, int32_t* proj, size_t stride, const uint8_t* a96);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_combine_kernel(size_t n, int32_t* proj, size_t stride);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_finish_kernel(size_t n, size_t L, const uint8_t* tr, const uint8_t* gsk97, const uint8_t* rnd224, const uint8_t* t49, const uint8_t* st_a, const uint8_t* st_pub, uint8_t* sig435, uint8_t* status, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) bbs04_issue_pack_kernel(size_t n, const uint8_t* a49, const uint8_t* x32, const uint8_t* st_pub, uint8_t* gsk97, int* bad_flag);
// k_ps.hip: PS signatures from the wire formats (msg_mode: ps.hpp PS_MSG_HASH / PS_MSG_ENCODE)
__global__ void __launch_bounds__(BLOCK, 2) ps_wire_prep_kernel(size_t n, size_t msg_len, int mode, size_t nmsg, const uint8_t* sig98, const uint8_t* msgs, uint8_t* s49, uint8_t* m32);
__global__ void __launch_bounds__(BLOCK, 2) ps_wire_finish_kernel(size_t n, size_t npub, const uint8_t* st_sig, const uint8_t* st_pub, uint8_t* ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ps_generator_kernel(uint8_t* out96);
__global__ void __launch_bounds__(BLOCK, 2) ps_sign_prep_kernel(size_t n, size_t nused, size_t msg_len, int mode, const uint8_t* x48, const uint8_t* y48, const uint8_t* msgs, const uint8_t* t32, uint8_t* sc, uint8_t* key_ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ps_sign_finish_kernel(size_t n, const uint8_t* key_ok, uint8_t* sig98);
__global__ void __launch_bounds__(BLOCK, 2) ps_randomize_prep_kernel(size_t n, const uint8_t* r32, uint8_t* sc);
__global__ void __launch_bounds__(BLOCK, 2) ps_randomize_finish_kernel(size_t n, const uint8_t* st, uint8_t* out98, uint8_t* status);
__global__ void __launch_bounds__(BLOCK, 2) ps_aggregate_finish_kernel(uint8_t* all_ok, const int* bad_flag);
// k_ac_bbs.hip: AC-bbs credential presentation and verification (ac_bbs.hpp; the base order travels by value)
struct ac_bbs_order;
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_key_kernel(size_t nattr, ac_bbs_order ord, const uint8_t* y49, uint8_t* out49);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_bcast96_kernel(size_t n, const uint8_t* src96, uint8_t* dst96);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_verify_prep_kernel(size_t n, size_t nI, size_t nJ, const uint8_t* pres243, const uint8_t* u48, const uint8_t* attr48, uint8_t* p49, uint8_t* sc3, uint8_t* sca, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_encode_kernel(size_t n, const uint8_t* a96, const uint8_t* b96, const uint8_t* u96, uint8_t* e49, uint8_t* q96);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_challenge_kernel(size_t n, size_t msg_len, const uint8_t* msgs, const uint8_t* e49, uint8_t* tr, uint8_t* c32);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_verify_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p, const uint8_t* r49, const uint8_t* u49, const uint8_t* okp, uint8_t* ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_pres_prep_kernel(size_t n, size_t nattr, size_t nJ, ac_bbs_order ord, const uint8_t* attr48, const uint8_t* sig97, const uint8_t* rnd, uint8_t* a49, uint8_t* sca, uint8_t* scd, uint8_t* sc2, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_pres_finish_kernel(size_t n, size_t nattr, size_t nJ, ac_bbs_order ord, const uint8_t* attr48, const uint8_t* sig97, const uint8_t* rnd, const uint8_t* e49, const uint8_t* c32, const uint8_t* st, const uint8_t* st_a, const uint8_t* st_pub, uint8_t* pres243, uint8_t* u48, uint8_t* status, int* bad_flag);
// k_ac_rbbs.hip: AC-rbbs credential redaction, presentation and verification (ac_rbbs.hpp; the index lists and the plan travel by value)
struct ac_rbbs_plan;
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_gather_kernel(size_t count, size_t rec_bytes, ac_bbs_order ord, const uint8_t* in, uint8_t* out);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_verify_prep_kernel(size_t n, size_t nI, ac_bbs_order idx, const uint8_t* pres341, const uint8_t* attr48, uint8_t* p49, uint8_t* sc3, uint8_t* sca, uint8_t* q32, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_encode_kernel(size_t n, size_t count, const uint8_t* p96, uint8_t* e49);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_challenge_kernel(size_t n, size_t msg_len, const uint8_t* msgs, const uint8_t* e49, int u_col, uint8_t* tr, uint8_t* c32);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_verify_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p, const uint8_t* r49, const uint8_t* u49, const uint8_t* ok1, const uint8_t* ok3, uint8_t* ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_pres_prep_kernel(size_t n, const uint8_t* sig97, const uint8_t* cache196, const uint8_t* rnd, uint8_t* p49, uint8_t* scr, uint8_t* sc2, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_pres_finish_kernel(size_t n, const uint8_t* sig97, const uint8_t* rnd, const uint8_t* e49, const uint8_t* c32, const uint8_t* st, const uint8_t* st_p, uint8_t* pres341, uint8_t* status);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_redact_prep_kernel(size_t n, ac_rbbs_plan pl, const uint8_t* attr48, const uint8_t* sig97, uint8_t* a49, uint8_t* sca, uint8_t* scw, uint8_t* aI48, uint8_t* q32, uint8_t* scd, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_redact_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_a, const uint8_t* o96, uint8_t* cache196, uint8_t* status, int* bad_flag);
// k_ac_rps.hip: AC-rps credential redaction, presentation and verification (ac_rps.hpp; the index list and the plan travel by value)
struct ac_rps_plan;
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_verify_prep_kernel(size_t n, size_t nI, const uint8_t* pres389, const uint8_t* attr48, uint8_t* p49, uint8_t* p97, uint8_t* sc2, uint8_t* sca, uint8_t* st, uint8_t* st_a);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_verify_q_kernel(size_t n, ac_rps_plan pl, const uint8_t* s1_49, const uint8_t* s2_49, const uint8_t* ts192, const uint8_t* attr48, uint8_t* pre, uint8_t* q32);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_verify_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_a, const uint8_t* st_p, const uint8_t* c32, const uint8_t* sc2, const uint8_t* okp, uint8_t* ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_pres_prep_kernel(size_t n, size_t nattr, const uint8_t* attr48, const uint8_t* sig195, const uint8_t* cache97, const uint8_t* usk48, const uint8_t* rnd, uint8_t* p49, uint8_t* p97, uint8_t* scr, uint8_t* sc2, uint8_t* scz, uint8_t* sct, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_pres_scalars_kernel(size_t n, ac_rps_plan pl, const uint8_t* s1_49, const uint8_t* s2_49, const uint8_t* ts97, const uint8_t* attr48, const uint8_t* rnd, uint8_t* pre, uint8_t* q32, uint8_t* sc3);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_pres_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p, const uint8_t* e49, const uint8_t* s3_49, const uint8_t* ts97, const uint8_t* c32, const uint8_t* usk48, const uint8_t* rnd, uint8_t* pres389, uint8_t* status, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_redact_prep_kernel(size_t n, size_t nattr, size_t nI, ac_bbs_order idx, const uint8_t* attr48, const uint8_t* sig195, uint8_t* p49, uint8_t* p97, uint8_t* sca, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_g2_sub_kernel(size_t n, const uint8_t* a192, const uint8_t* b192, uint8_t* out, int fmt, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_redact_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p, const uint8_t* h97, uint8_t* cache97, uint8_t* status, int* bad_flag);
// k_mhac_bbs.hip: MHAC-bbs credential presentation and verification (mhac_bbs.hpp; the index sets travel by value)
struct mhac_bbs_sets;
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_verify_prep_kernel(size_t n, size_t nz, size_t nhp, size_t nrp, const uint8_t* crev49, const uint8_t* fixed242, const uint8_t* z48, const uint8_t* zhp48, const uint8_t* pub48, uint8_t* p49, uint8_t* sc3, uint8_t* sca, uint8_t* c32, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_verify_finish_kernel(size_t n, size_t nrp, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p, const uint8_t* p96, const uint8_t* u49, const uint8_t* pub48, const uint8_t* c32, const uint8_t* okp, uint8_t* tr, uint8_t* ok, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_pres_prep_kernel(size_t n, size_t t, mhac_bbs_sets s, const uint8_t* A49, const uint8_t* D49, const uint8_t* crev49, const uint8_t* cpub49, const uint8_t* lam48, const uint8_t* eshare48, const uint8_t* ashare48, const uint8_t* pub48, const uint8_t* rnd, uint8_t* p49, uint8_t* scr, uint8_t* scu, uint8_t* sch, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_pres_finish_kernel(size_t n, size_t t, mhac_bbs_sets s, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p, const uint8_t* o96, const uint8_t* u96, const uint8_t* lam48, const uint8_t* eshare48, const uint8_t* ashare48, const uint8_t* pub48, const uint8_t* rnd, uint8_t* tr, uint8_t* fixed242, uint8_t* z48, uint8_t* zhp48, uint8_t* status, int* bad_flag);
// k_mhac_iss.hip: MHAC-bbs attribute generation, issuance, group and type (mhac_iss.hpp; the sets, S, lambda and the type plan travel by value)
struct mhac_iss_lambda;
struct mhac_iss_parties_set;
struct mhac_iss_type_plan;
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_attr_kernel(size_t k, size_t np, size_t t, mhac_bbs_sets s, const uint8_t* rnd, uint8_t* pub48, uint8_t* ashare48, uint8_t* sc);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_attr_finish_kernel(size_t L, size_t np, size_t nPrv, size_t nPub, size_t npub, const uint8_t* st_pub, uint8_t* pub48, uint8_t* ashare48, uint8_t* C49, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_iss_prep_kernel(size_t k, size_t np, size_t t, size_t nPub, mhac_iss_lambda lam, const uint8_t* sk48, const uint8_t* pub48, const uint8_t* rnd, uint8_t* gam, uint8_t* st, uint8_t* e32, uint8_t* scl, uint8_t* scp, uint8_t* nes, uint8_t* eshare48, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_cols_kernel(size_t k, size_t np, size_t t, const uint8_t* c96, uint8_t* q96);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_rep_kernel(size_t L, size_t np, const uint8_t* a96, uint8_t* r96);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_iss_finish_kernel(size_t L, size_t np, size_t npub, const uint8_t* st_pub, const uint8_t* gam, const uint8_t* st, const uint8_t* st_c, const uint8_t* a96, const uint8_t* w96, uint8_t* A49, uint8_t* eshare48, uint8_t* D49, uint8_t* status, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_group_prep_kernel(size_t n, size_t np, size_t t, size_t nPrv, mhac_iss_parties_set S, mhac_iss_lambda lam, const uint8_t* D49, const uint8_t* eshare48, const uint8_t* ashare48, uint8_t* p49, uint8_t* sc, uint8_t* lam48, uint8_t* eS48, uint8_t* aS48);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_group_finish_kernel(size_t n, size_t t, size_t nPrv, const uint8_t* st_p, const uint8_t* u96, uint8_t* Dg49, uint8_t* lam48, uint8_t* eS48, uint8_t* aS48, uint8_t* status);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_type_prep_kernel(size_t n, size_t nPub, mhac_iss_type_plan plan, const uint8_t* pub48, uint8_t* sca, uint8_t* st);
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_type_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* r96, const uint8_t* p96, uint8_t* crev49, uint8_t* cpub49, uint8_t* status, int* bad_flag);
// k_ac_issue.hip: AC-bbs / AC-rbbs / AC-rps credential issuance and AC-rps user_keygen (ac_issue.hpp)
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_bbs_prep_kernel(size_t n, size_t nattr, size_t nsk, const uint8_t* sk48, const uint8_t* attr48, const uint8_t* rnd32, uint8_t* sca, uint8_t* w32, uint8_t* d32, uint8_t* st, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_bbs_finish_kernel(size_t n, size_t npub, size_t nsk, const uint8_t* st_pub, const uint8_t* sk48, const uint8_t* st, const uint8_t* a96, const uint8_t* w32, uint8_t* sig97, uint8_t* status, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_keygen_prep_kernel(size_t n, const uint8_t* rnd32, uint8_t* sc);
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_keygen_finish_kernel(size_t n, const uint8_t* st_pub, const uint8_t* sc, uint8_t* usk48, uint8_t* upk49, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_rps_prep_kernel(size_t n, size_t nattr, const uint8_t* sk96, const uint8_t* attr48, const uint8_t* rnd32, uint8_t* sca, uint8_t* al32, uint8_t* sc2, uint8_t* st, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_rps_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* sk96, const uint8_t* st, const uint8_t* st_z, const uint8_t* e49, const uint8_t* tm97, uint8_t* sig195, uint8_t* status, int* bad_flag);
// k_fixed.hip: device-built tables in arrays of 1 .. TABLE_ARRAY_MAX, tab_stride dwords apart; the cached points travel by value
constexpr int TABLE_ARRAY_MAX = 32;
struct table_points { const uint8_t* p[TABLE_ARRAY_MAX]; };
__global__ void __launch_bounds__(64, 1) fixed_cache_check_kernel(table_points pts, int nbytes, int32_t* tabs, int tab_stride);
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_tables_kernel(const uint8_t* bases96, int32_t* tabs, int tab_stride);
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_eval_kernel(size_t n, const int32_t* buf, const uint8_t* scalars, int32_t* proj, size_t proj_stride, size_t proj_off);
// per-lane sums over a set of shared G1 bases (C12381_G1_FIXED_SUM_MAX = G1_FIXED_SUM_MAX): nb tables behind one gate
constexpr int G1_FIXED_SUM_MAX = TABLE_ARRAY_MAX;
__global__ void __launch_bounds__(64, 1) g1_fixed_sum_gate_kernel(int nb, const uint8_t* bases96, const uint8_t* addend96, int32_t* gate, const int32_t* tabs, int tab_stride, int use_tables, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_sum_kernel(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride, const uint8_t* scalars, const uint8_t* addend96, int32_t* proj, size_t proj_stride);
__global__ void __launch_bounds__(BLOCK, 2) g1_fixed_sum_fold_kernel(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off, int has_col, int last, const uint8_t* addend96);
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_tables_kernel(const uint8_t* bases192, int32_t* tabs, int tab_stride);
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_eval_kernel(size_t n, const int32_t* buf, const uint8_t* scalars, const uint8_t* addend192, uint8_t* out, int fmt, int* bad_flag, int32_t* proj, size_t proj_stride);
// per-lane sums over a set of shared G2 bases (C12381_G2_FIXED_SUM_MAX = G2_FIXED_SUM_MAX): nb tables behind one gate, as the G1 form
constexpr int G2_FIXED_SUM_MAX = TABLE_ARRAY_MAX;
__global__ void __launch_bounds__(64, 1) g2_fixed_sum_gate_kernel(int nb, const uint8_t* bases192, const uint8_t* addend192, int32_t* gate, const int32_t* tabs, int tab_stride, int use_tables, int* bad_flag);
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_sum_kernel(size_t n, int nb, const int32_t* gate, const int32_t* tabs, int tab_stride, const uint8_t* scalars, const uint8_t* addend192, int32_t* proj, size_t proj_stride);
__global__ void __launch_bounds__(BLOCK, 2) g2_fixed_sum_fold_kernel(size_t n, const int32_t* gate, int32_t* proj, size_t proj_stride, size_t col_off, int has_col, int last, const uint8_t* addend192);

}  // namespace c12381
