// The spread acting forward's kernels (act_spread.h), a translation unit and
// so a code object of their own: the code objects of the training step's
// kernels stay byte for byte what they were (DESIGN.md section 3 "One Snake
// environment": moving kernels cost the flagship step 0.5-1 %; included at the
// end of kernels.hip these three cost it 0.15 %).
#include "kernels.h"
#include "act_spread.h"
