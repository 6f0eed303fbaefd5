// The attentions of two towers as one launch (attention.hip); used by block_forward (encoders.hip) and cmh_attention_pair.
#pragma once

#include "cmh_common.h"

namespace cmh {

// one side of the pair: the arguments of launch_attention_varlen
struct AttnProblem {
  const void* qkv;
  void* o;
  int dt, B, T, d, causal;
  const uint8_t* kpm;
  const int32_t* seq_off;
  float o8_inv_scale;
};

// bf16 MFMA forms only, each side T <= 80.  0 = launched; 1 = not a pair there is a kernel for (other dtype, T > 80, a pair of
// key-tile counts that is not instantiated, or CMH_PAIR_KERNELS=0): nothing was launched, the caller launches the two singly;
// < 0 = the launch itself failed
int launch_attention_pair(const AttnProblem& p0, const AttnProblem& p1, hipStream_t st);

// whether block_forward routes a two-tower layer's attentions through launch_attention_pair (CMH_ATTN_PAIR)
bool attention_pair_routed();

}  // namespace cmh
