// What BOTH channel-mixing kernel families use - K8 (channel_mix.hip: forward / input gradient) and K9 (channel_wgrad.hip: weight
// gradient): the GELU on the staging path and the three-piece bfloat16 split of the K8-S / K9-S forms.  Helpers of one family only
// live in that family's file.
#pragma once
#include "uno_common.h"

namespace uno {

// exact-erf GELU (F.gelu default) and its derivative, for the fused forms: x := gelu(x) while a chunk goes to LDS
// (`act_in`: the layer consumes the activation of a tensor that is kept pre-activation) and y := (W x) * gelu'(pre) in the
// epilogue (`dgelu_of`: the input gradient of such a layer, handed back as the gradient of the pre-activation tensor)
__device__ __forceinline__ float cm_gelu(float x) { return uno_gelu(x); }
__device__ __forceinline__ float4 cm_gelu4(float4 v) { return make_float4(cm_gelu(v.x), cm_gelu(v.y), cm_gelu(v.z), cm_gelu(v.w)); }

// bf16 MFMA operands of the split forms (K8-S: channel_mix.hip; K9-S: channel_wgrad.hip): eight bf16 per lane as four dwords
typedef __bf16 cms_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned cms_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 cms_mfma(const cms_u32x4& a, const cms_u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cms_bf16x8, a), __builtin_bit_cast(cms_bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ void cms_split3(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = bf16_pack2(a, b);
    const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
    m = bf16_pack2(ra, rb);
    const float sa = ra - __uint_as_float(m << 16), sb = rb - __uint_as_float(m & 0xffff0000u);
    l = bf16_pack2(sa, sb);
}

}  // namespace uno
