// The launch layer of the string kernels: every launcher and workspace-size function that one of
// the string files (lev_*.hip, bitpar_classify.hip, oc_*.hip) defines for another file to call.
// pdt_api.hip and each defining file include it, so a signature that changes on one side only
// fails to compile.
#pragma once
#include "lev_common.hpp"

namespace pdt {

struct BitparArgs;  // bitpar_classify.hpp

// lev_skewed.hip, lev_rowsync.hip: the cell-by-cell recurrences
int launch_lev_skewed(LevArgs a, hipStream_t stream);
int launch_lev_rowsync(LevArgs a, bool exact, hipStream_t stream);

// bitpar_classify.hip, lev_bitpar.hip, oc_bitpar.hip: unit costs, bit-parallel (plan_bitpar: lev_common.hpp)
int launch_bitpar_classify(const BitparArgs &a, const BitparPlan &p, hipStream_t stream);
int launch_lev_bitpar(const LevArgs &la, const BitparPlan &p, void *ws, hipStream_t stream, LevTables tables);
int launch_oc_mask_bitpar(const LevArgs &a, void *ws, int64_t ws_bytes, hipStream_t stream);
int64_t oc_bitpar_workspace_bytes(int64_t R, int64_t H, int64_t N);
size_t oc_fused_lds_bytes(int64_t X, int64_t Y);

// lev_generic.hip: one workgroup per utterance, rows in the workspace -- distances and masks for
// references beyond 2 048 tokens
int launch_lev_workgroup(const LevArgs &a, bool inexact, void *ws, int64_t ws_bytes, hipStream_t stream);
int64_t lev_workgroup_ws_per_utt(int64_t R, int64_t H, int *P_out);
int launch_oc_expand_generic(const uint32_t *bitmask, const int64_t *class_tokens, int R, int Hout,
                             int64_t N, int C, int64_t padding, int64_t *targets, int64_t tgt_sh,
                             int64_t tgt_sn, hipStream_t stream);

// oc_expand.hip: class bitmasks -> padded token lists, references of up to 2 048 tokens
int launch_oc_expand(const uint32_t *bitmask, const int64_t *class_tokens, int R, int Hout,
                     int64_t N, int C, int64_t padding, int64_t *targets, int64_t tgt_sh,
                     int64_t tgt_sn, hipStream_t stream);

}  // namespace pdt
