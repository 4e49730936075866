// constrained.hip — the label-constrained variant of the greedy decode tail (include/icl_hip.h, "K11 (constrained)").
//
// One block per sequence, three block-uniform cases:
//   finished row     pad, log-prob 0, state untouched (argmax_eos_kernel's rule);
//   free row         (state -1, or a state id outside the automaton) argmax_eos_kernel's token — lowest index on ties, a NaN
//                    logit cannot be chosen — and its log-probability under the softmax of the whole row;
//   constrained row  the outgoing edges of the row's state whose target can still reach an accepting state inside the remaining
//                    budget are the candidates; the token is the best of them and the log-probability is taken over them only.
// Both live cases are ONE pass: every lane keeps (running maximum, sum of exp(x - maximum), index of the maximum) over its
// share — the online soft-max recurrence — and the 256 triples are merged by shuffles and 4 LDS slots.  A free row reads its
// 4*V bytes once (argmax_eos_kernel's traffic); a constrained row reads the edge list of one state and one logit per edge.
// Plain dword loads and stores only; no allocation, no synchronisation with the host, nothing that a stream capture refuses.
#include "common.h"

struct MaxSum {
  float m;      // running maximum
  float s;      // sum of exp(x - m) over the values seen that are > -inf
  int i;        // index of the first value equal to m in index order; 0x7fffffff = nothing seen
};

__device__ __forceinline__ void maxsum_push(MaxSum& a, float x, int idx) {      // x is not NaN
  if (x > a.m) {                                  // a.m = -inf at first: expf(-inf) = 0 clears the empty sum
    a.s = a.s * expf(a.m - x) + 1.0f;
    a.m = x;
    a.i = idx;
  } else {
    if (x > -INFINITY) a.s += expf(x - a.m);      // here a.m >= x > -inf: the difference is defined
    if (x == a.m && idx < a.i) a.i = idx;         // all -inf so far: the first index offered wins
  }
}

__device__ __forceinline__ void maxsum_merge(MaxSum& a, float m, float s, int i) {
  if (m > a.m || (m == a.m && i < a.i)) {
    const float t = a.m; a.m = m; m = t;
    const float u = a.s; a.s = s; s = u;
    a.i = i;
  }
  if (m > -INFINITY) a.s += s * expf(m - a.m);    // the smaller side, rescaled; an all -inf side holds no mass
}

__global__ __launch_bounds__(256) void argmax_fsm_kernel(
    const float* logits, int64_t ldl, int V, const int* state_off, const int* edge_tok, const int* edge_next,
    const int* state_dist, int n_states, int n_edges, int* state, int steps_left, int eos_id, int eos_id2, int pad_id,
    int* finished, int* out_tokens, int out_stride, int step, int* next_ids, float* out_logprob) {
  __shared__ float sm[4], ss[4];
  __shared__ int si[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t out = (int64_t)b * out_stride + step;
  if (finished[b]) {                              // block-uniform: every thread reads the same word
    if (tid == 0) {
      out_tokens[out] = pad_id;
      next_ids[b] = pad_id;
      if (out_logprob) out_logprob[out] = 0.0f;
    }
    return;
  }
  const float* row = logits + (int64_t)b * ldl;
  const int st = state[b];
  const bool constrained = st >= 0 && st < n_states;
  MaxSum a = {-INFINITY, 0.0f, 0x7fffffff};
  if (constrained) {
    // the tables were validated by the host before the upload; the clamps below only keep a mistaken table inside its arrays
    const int e0 = max(0, state_off[st]), e1 = min(n_edges, state_off[st + 1]);
    for (int e = e0 + tid; e < e1; e += 256) {
      const int tok = edge_tok[e], nx = edge_next[e];
      if ((unsigned)tok < (unsigned)V && (unsigned)nx < (unsigned)n_states && state_dist[nx] <= steps_left - 1) {
        const float x = row[tok];
        maxsum_push(a, x == x ? x : -INFINITY, e);            // a NaN candidate is a -inf candidate: it keeps its place
      }
    }
  } else {
    for (int v = tid; v < V; v += 256) {
      const float x = row[v];
      if (x == x) maxsum_push(a, x, v);                       // a NaN logit cannot be chosen and carries no mass
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(a.m, o, 64), os = __shfl_xor(a.s, o, 64);
    const int oi = __shfl_xor(a.i, o, 64);
    maxsum_merge(a, om, os, oi);
  }
  if ((tid & 63) == 0) {
    sm[tid >> 6] = a.m;
    ss[tid >> 6] = a.s;
    si[tid >> 6] = a.i;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) maxsum_merge(a, sm[w], ss[w], si[w]);
    int tok, fin = 0;
    float lp;
    if (constrained && a.i == 0x7fffffff) {       // no candidate: the caller broke steps_left >= state_dist[state]; end the row
      tok = pad_id;
      fin = 1;
      lp = __uint_as_float(0x7fc00000u);
    } else {
      float x;
      if (constrained) {
        tok = edge_tok[a.i];
        state[b] = edge_next[a.i];
        x = row[tok];
      } else {
        tok = a.i == 0x7fffffff ? 0 : a.i;        // all-NaN row: keep a valid id, as argmax_eos_kernel does
        x = row[tok];
      }
      if (x != x) x = -INFINITY;
      lp = (x - a.m) - logf(a.s);                 // NaN when no candidate is finite (m = -inf) or one is +inf: no distribution
    }
    if (tok == eos_id || tok == eos_id2) fin = 1;
    finished[b] = fin;
    out_tokens[out] = tok;
    next_ids[b] = tok;
    if (out_logprob) out_logprob[out] = lp;
  }
}

extern "C" int icl_argmax_fsm(const float* logits, int64_t ldl, int32_t B, int32_t V, const int32_t* state_off,
                              const int32_t* edge_tok, const int32_t* edge_next, const int32_t* state_dist, int32_t n_states,
                              int32_t n_edges, int32_t* state, int32_t steps_left, int32_t eos_id, int32_t eos_id2,
                              int32_t pad_id, int32_t* finished, int32_t* out_tokens, int32_t out_stride, int32_t step,
                              int32_t* next_ids, float* out_logprob, void* stream) {
  ICL_CHECK_ARG(logits && finished && out_tokens && next_ids && state, "icl_argmax_fsm: NULL pointer");
  ICL_CHECK_ARG(state_off && edge_tok && edge_next && state_dist, "icl_argmax_fsm: NULL automaton table");
  ICL_CHECK_ARG(B > 0 && V > 0 && ldl >= V, "icl_argmax_fsm: bad sizes");
  ICL_CHECK_ARG(n_states >= 1 && n_edges >= 1, "icl_argmax_fsm: empty automaton (n_states=%d, n_edges=%d)", n_states, n_edges);
  ICL_CHECK_ARG(steps_left >= 1, "icl_argmax_fsm: steps_left=%d must be >= 1", steps_left);
  ICL_CHECK_ARG(step >= 0 && step < out_stride, "icl_argmax_fsm: step=%d outside out_stride=%d", step, out_stride);
  hipLaunchKernelGGL(argmax_fsm_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, state_off, edge_tok,
                     edge_next, state_dist, n_states, n_edges, state, steps_left, eos_id, eos_id2, pad_id, finished,
                     out_tokens, out_stride, step, next_ids, out_logprob);
  ICL_CHECK_LAUNCH("icl_argmax_fsm");
  return ICL_OK;
}
