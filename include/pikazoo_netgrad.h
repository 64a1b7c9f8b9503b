/* pikazoo_netgrad.h -- C ABI of libpikazoo_netgrad.so: the backward pass of pikazoo_net.h's three-layer policy net, from
 * d loss / d head (the [n, out_features] tensor that pz_ppo_loss writes) to the six parameter gradients, in ONE call.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path, pikazoo_amd.learn, pikazoo_amd.policy,
 * pikazoo_amd.ppo or pikazoo_amd.net loads it.  Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2,
 * PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of a launch).
 *
 * Pointers are caller-owned device memory; two launches on `stream` whatever n is, no allocation, no synchronisation:
 * graph-capturable.  The parameters are read in place by every call or replay.
 *
 * THE DEFINITION.  Per row x of an agent, in float32, with the forward recomputed inside the call (no saved activations;
 * nothing is read but obs, the parameters and grad_head):
 *     z1 = W1 x + b1;  h1 = act(z1);  z2 = W2 h1 + b2;  h2 = act(z2)                       (pikazoo_net.h's definition)
 *     d3 = the row of grad_head
 *     d2 = (W3^T d3) * act'(z2);     d1 = (W2^T d2) * act'(z1)
 *     tanh: act'(z) = 1 - h^2        relu: act'(z) = (z <= 0) ? 0 : 1     (0 at z == 0, as torch; 1 for a NaN z)
 *     dW3 = sum_rows d3 h2^T   db3 = sum_rows d3
 *     dW2 = sum_rows d2 h1^T   db2 = sum_rows d2
 *     dW1 = sum_rows d1 x^T    db1 = sum_rows d1
 * The derivative is a FACTOR: a NaN or an infinity in W^T d times 0 is NaN.  There is no gradient with respect to the
 * observations.
 * WHAT A NaN REACHES follows from these lines and nothing else.  A NaN in one row's grad_head[c] makes db3[c], dW3[c, :] and
 * every gradient of layers 1 and 2 NaN; the other rows of dW3 and db3 do not see it.  A NaN observation x[k] makes that row's
 * z1, h1, z2 and h2 NaN, so dW3 and dW2 are NaN throughout; db3 = sum d3 never sees it.  Under tanh act' is NaN too, and
 * db2, dW1 and db1 are NaN.  Under relu a NaN z passes the gradient on (factor 1), so d2 and d1 of that row stay finite: db2
 * and db1 stay finite and of dW1 only column k is NaN.
 *
 * OBSERVATIONS and PARAMETERS: as pz_mlp_forward takes them (all five formats of pz_net_obs_format, obs_pitch in elements;
 * torch's own nn.Linear tensors, float32, contiguous).  GRAD_HEAD: n rows of out_features elements at grad_pitch ELEMENTS, of
 * grad_format (pz_net_out_format's values).  Pad columns of obs and grad_head and the memory behind row n-1 never reach the
 * arithmetic; a row >= n contributes +0 to every sum.
 *
 * OUTPUTS: six contiguous float32 tensors per agent with the parameters' shapes.  They are OVERWRITTEN, not accumulated
 * into, and must not alias an input, the workspace or each other.
 *
 * TWO AGENTS.  Agent 2's obs, six parameters and grad_head are ALL NULL or ALL non-NULL.  When they are present:
 *   - agent 2's six gradient pointers all non-NULL: each agent gets gradients of its own;
 *   - all six NULL: a SHARED net.  Agent 2's parameter pointers must equal agent 1's (else PZ_E_CONFIG); agent 1's outputs
 *     receive (agent 1's sum) + (agent 2's sum), in that order.
 * A mix of NULL and non-NULL, or gradient pointers of an absent agent 2, is PZ_E_NULL.
 *
 * SIZES: pz_mlp_forward's box: 1 <= in_features <= 72, hidden in {32, 64, 128}, 1 <= out_features <= 40, 0 <= n <= 2^30,
 * obs_pitch >= in_features, grad_pitch >= out_features.
 *
 * ARITHMETIC: operands and accumulation are float32 (v_mfma_f32_32x32x2_f32: a chain of fused multiply-adds, one rounding per
 * product); nothing is rounded to a narrower format.  tanh is pikazoo_net.h's.
 *
 * THE REDUCTIONS ARE DETERMINISTIC, as pikazoo_ppo.h states it.  No floating-point atomic accumulates anything.  A workgroup
 * takes the passes (128 / hidden * 32 consecutive rows each) p = b, b + B, b + 2 B, ... of its agent in that order, B being
 * the number of workgroups per agent: min(number of passes, compute units of the device).  It writes its partial sums into
 * `workspace` with plain stores; a second, small launch on the same stream sums the partials in the order of their index
 * (and, for a shared net, agent 2's total onto agent 1's).  Two calls on the same inputs with the same n on the same device
 * return equal bits, whatever the workspace held before; with separate gradients agent 1's bits do not depend on agent 2's
 * presence, nor on the pitches, the base offsets or the formats of tensors holding the same values.  What the bits MAY
 * depend on: n (it sets the number of passes and so which rows share a partial sum) and the grid cap B taken from the
 * device's compute-unit count.
 *
 * WORKSPACE: caller-owned scratch of pz_mlp_backward_workspace_bytes(...) bytes, aligned to 16 bytes, never shared by two
 * calls in flight.  Nothing is written behind those bytes.
 *
 * Checked before any launch, in this order:
 *   PZ_E_NULL    obs, a parameter, grad_head, a gradient output of agent 1 or workspace is NULL; agent 2's pointers mixed;
 *   PZ_E_SIZE    a size outside the box, a pitch below its width, n * pitch * 4 bytes beyond int64;
 *   PZ_E_CONFIG  an unknown format or activation; a shared net whose agent 2 parameter pointers differ from agent 1's;
 *   PZ_E_ALIGN   a pointer not aligned to its element (observations and grad_head 4 or 2 bytes, parameters and gradients
 *                4), the workspace not aligned to 16.
 * n == 0 returns PZ_OK without a launch and writes nothing.
 */
#ifndef PIKAZOO_NETGRAD_H
#define PIKAZOO_NETGRAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_NETGRAD_ABI_VERSION 1

int pz_netgrad_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_netgrad_build_id(void);

/* bytes of scratch pz_mlp_backward needs for n rows of one or both agents on the current device; 0 for arguments outside the
 * box (n <= 0 included) */
int64_t pz_mlp_backward_workspace_bytes(int64_t n, int32_t in_features, int32_t hidden, int32_t out_features);

int pz_mlp_backward(const void *obs_p1, const void *obs_p2, int32_t obs_format, int64_t n, int32_t in_features,
                    int64_t obs_pitch, int32_t hidden, int32_t out_features, int32_t activation, const float *w1_p1,
                    const float *b1_p1, const float *w2_p1, const float *b2_p1, const float *w3_p1, const float *b3_p1,
                    const float *w1_p2, const float *b1_p2, const float *w2_p2, const float *b2_p2, const float *w3_p2,
                    const float *b3_p2, const void *grad_head_p1, const void *grad_head_p2, int32_t grad_format,
                    int64_t grad_pitch, float *dw1_p1, float *db1_p1, float *dw2_p1, float *db2_p1, float *dw3_p1,
                    float *db3_p1, float *dw1_p2, float *db1_p2, float *dw2_p2, float *db2_p2, float *dw3_p2, float *db3_p2,
                    void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_NETGRAD_H */
