// pm_kernel_rp_occ4.hip - the row-pair kernel (pm_kernel_rp.inc) compiled for the launches whose LDS footprint fits FOUR
// workgroups per CU (slot groups, window pitches 104 and 112: borders 20 and 21): 128 VGPRs, 256 threads.  A translation unit
// of its own - see SID_PM_OCC at the top of pm_kernel_base.h.
#define SID_PM_OCC 4
#include "pm_kernel_rp.inc"

namespace sid {

// the only export of the second compilation: its kernels (the rows with occ = 4 of SID_PM_RP_INSTANCES)
PmKernel rp_occ4_kernel(int img_size, int paired, int pitch) { return rp_kernel<4>(img_size, 4, paired, pitch, false); }

}  // namespace sid
