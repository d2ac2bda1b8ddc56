// Every run-time switch of libpdt_amd.so in one place.  The PDT_* environment variables are read
// ONCE, the first time an entry point asks (no getenv on a launch path); pdt_amd_set_switch /
// pdt_amd_get_switch (include/pdt_amd.h) change / read one afterwards -- that is how the tests run two
// routes in one process.  The table of names is in INTEGRATION.md ("Switches").
#pragma once

namespace pdt {

struct Switches {
  int lev_bitpar;      // PDT_LEV_BITPAR     1  bit-parallel distance kernels for unit costs (0: cell-by-cell kernels)
  int oc_bitpar;       // PDT_OC_BITPAR      1  bit-parallel optimal-completion mask (0: row-synchronous kernel)
  int ctc_exact_div;   // PDT_CTC_EXACT_DIV  0  probabilities as the IEEE quotient e / sum (1) instead of e * (1 / sum)
  int ctc_rowreg;      // PDT_CTC_ROWREG     1  rows of 320+ tokens of the CTC search held in the producers' registers (0: LDS ring of rows; 2: from 128 tokens)
  int step_wide;       // PDT_STEP_WIDE      0  step functions always on the radix-select kernels (1)
  int ctc_pair;        // PDT_CTC_PAIR       1  CTC search at V = 256, W = 16: the producer takes two frames per pass, one per half wave (0: one; same bits)
  int step_flat;       // PDT_STEP_FLAT      1  step functions: one selection over all K' * V candidates (beam) / one list for prefixes that share
                       //                       their extension row (CTC) (0: a sorted list per prefix; same results)
  int ctc_lean_extra;  // PDT_CTC_LEAN_EXTRA 1  CTC frame: one-prefix and tie frames decided beside the lean tier (0: by the full tiers, same results)
  int ctc_steady;      // PDT_CTC_STEADY     1  CTC search without a model: frames whose best extensions are in rank order and beat everything
                       //                       else skip the lean tier's sort (0: every lean frame sorts; same kernel instance, same bits)
  int ctc_twoframe;    // PDT_CTC_TWOFRAME   1  ... at V = 256, W = 16: two steady frames of a producer pass decided at once, one per 16-lane row
                       //                       (0: frame by frame; same kernel instance, same bits; PDT_CTC_STEADY=0 implies 0)
  int ctc_pace;        // PDT_CTC_PACE       1  CTC search, one-producer forms: a producer's issue priority steps down with its progress, so the
                       //                       utterances of a launch end together (0: fixed priorities; same kernel instance, same bits)
};

Switches &switches();

}  // namespace pdt
