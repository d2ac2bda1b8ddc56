// The float16 instances of the CTC prefix search over long rows held in registers (ctc_rowreg.hip:
// the kernel and its launch table, compiled here for this element type alone, so that the float32, float16 and
// bfloat16 sets build side by side).
#define PDT_ROWREG_ELEM f16_t
#define PDT_ROWREG_ELEM_LAUNCH launch_ctc_rowreg_f16
#include "ctc_rowreg.hip"
