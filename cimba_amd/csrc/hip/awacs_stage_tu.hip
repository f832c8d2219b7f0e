// Stage-test translation unit of the AWACS kernels: awacs_kernel.hip built
// a second time with only its device functions, the beamforming check
// kernels and the stage-test kernels and entry points (the
// CIMBA_AWACS_STAGE_TU blocks there).  Nothing here is on the production
// path; keeping it out of the production unit leaves awacs_kernel and
// awacs_block_kernel compiled exactly as before.
#define CIMBA_AWACS_STAGE_TU 1
#include "awacs_kernel.hip"
