// shared_attn_fwd_pipe_ragged.hip - the per-reference-count instantiations of the software-pipelined 32-row kernel (WithRefCounts of
// the PRESC and EARLYQK forms x fold x seg_mass; shared_attn_fwd_pipe.hip has the kernel and says what the form does) and the
// combine of their K/V-range pieces.  An object of their own, as the key-bias forms have: the instantiations of
// shared_attn_fwd_pipe.o and shared_attn_fwd_pipe_bias.o stay the ones they were, compiled from the code they were compiled from.
#define IR_PIPE_RAGGED_TU 1
#include "shared_attn_fwd_pipe.hip"
