// bpgpu_internal.h -- what the translation units of libbpgpu.so share beside the public header: not exported.
#ifndef BPGPU_INTERNAL_H
#define BPGPU_INTERNAL_H
#include "../../include/bpgpu.h"

extern "C" {
// bpgpu_r1cs_verify_stream with the choice of its operand route handed in.  in_place_ok != 0: the public call's behaviour --
// page-locked operands are fetched in place over the bus (k_fetch3), pageable ones take the staged copies.  in_place_ok == 0: staged
// copies whatever the memory is.  bpgpu_pool.hip decides per slot: a device must not read host memory that is not mapped for it.
__attribute__((visibility("hidden"))) int bpgpu_internal_verify_stream(bpgpu_ctx *ctx, const bpgpu_gens *g, const bpgpu_circuit *c, size_t nb,
                                                                       size_t n1, size_t k, const uint8_t *points, const uint8_t *scalars,
                                                                       const uint8_t *challenges, int32_t *ok, int in_place_ok);
}
#endif
