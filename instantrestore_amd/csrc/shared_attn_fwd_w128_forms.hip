// shared_attn_fwd_w128_forms.hip - the valid_refs / seg_mass instantiations of the 128-rows-per-wave kernel (FORMS = true;
// shared_attn_fwd_w128.hip has the kernel and says what the forms do).  An object of their own: the <T, FOLD> kernels of the
// default dispatch stay the only four in shared_attn_fwd_w128.o, compiled from exactly the code they were, and the build guards
// (tools/check_resources.py, tests/test_build_guards.py, tests/test_w128_forms_cpu.py) hold both objects to the same rules.
#define IR_W128_FORMS 1
#include "shared_attn_fwd_w128.hip"
