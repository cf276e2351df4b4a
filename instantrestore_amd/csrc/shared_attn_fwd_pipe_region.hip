// shared_attn_fwd_pipe_region.hip - the region instantiations of the software-pipelined 32-row kernel (WithRegions of the PRESC and
// EARLYQK forms x fold x seg_mass; shared_attn_fwd_pipe.hip has the kernel and says what the form does) and the combine of their
// K/V-range pieces.  An object of their own: the instantiations of the other objects stay the ones they were, compiled from the
// code they were compiled from.
#define IR_PIPE_REGION_TU 1
#include "shared_attn_fwd_pipe.hip"
