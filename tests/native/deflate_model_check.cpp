// CPU harness: the host half of the device DEFLATE encoder's residual-stream table (pyrecode_amd/csrc/rc_deflate_model.h) behind a C
// entry point, so that tests/test_deflate_values_cpu.py can compare it with the serial model (tests/deflate_values_model.py).
#include "../../pyrecode_amd/csrc/rc_deflate_model.h"

extern "C" int deflate_model_check(const uint32_t *hist256, uint8_t *len257, uint16_t *code257, uint8_t *hdr, uint32_t hdr_cap,
                                   uint32_t *hdr_bits, uint32_t *usable)
{
    rc::DeflateModel M;
    rc::dm_build_model(hist256, &M, len257);
    for (int s = 0; s < rc::DM_SYMS; ++s) code257[s] = M.code[s];
    if (hdr_cap < sizeof M.hdr) return -1;
    memcpy(hdr, M.hdr, sizeof M.hdr);
    *hdr_bits = M.hdr_bits;
    *usable = M.usable;
    return 0;
}
