// The rules of a multi-categorical head (include/agx_multi.h), for the policy
// step (multi_policy.hip) and the fused learner (graph_learner.hip): K >= 1
// components of n_k >= 1 choices, L = sum n_k logits, L == net->n_actions.
// `who` names the entry point in errors.
#pragma once

#include "../../include/agx_graph.h"
#include "../../include/agx_multi.h"
#include "agx_common.h"

namespace agx {
namespace {

// K, nvec and L = sum nvec of a head -> L, or -1 with the error set
int head_width(const agx_multi_head &h, const char *who) {
    if (h.K < 1 || h.K > AGX_PPO_GRAPH_MAX_ACTIONS) {
        set_error("%s: %d components (1..%d)", who, h.K, AGX_PPO_GRAPH_MAX_ACTIONS);
        return -1;
    }
    int L = 0;
    for (int k = 0; k < h.K; ++k) {
        if (h.nvec[k] < 1 || h.nvec[k] > AGX_PPO_GRAPH_MAX_ACTIONS) {
            set_error("%s: component %d has %d choices (1..%d)", who, k, h.nvec[k], AGX_PPO_GRAPH_MAX_ACTIONS);
            return -1;
        }
        L += h.nvec[k];
    }
    if (L > AGX_PPO_GRAPH_MAX_ACTIONS) {
        set_error("%s: %d logits (1..%d)", who, L, AGX_PPO_GRAPH_MAX_ACTIONS);
        return -1;
    }
    return L;
}

// the head's L logits (head_width) are the actor's output
int head_fits(const agx_ppo_graph *net, int L, const char *who) {
    AGX_REQUIRE(L == net->n_actions, "%s: nvec sums to %d, the actor's output has %d logits", who, L, net->n_actions);
    return AGX_OK;
}

// head with the components past K zeroed (they are never read): what the kernels take by value
agx_multi_head head_arg(const agx_multi_head &head) {
    agx_multi_head h{};
    h.K = head.K;
    for (int k = 0; k < head.K; ++k) h.nvec[k] = head.nvec[k];
    return h;
}

}  // namespace
}  // namespace agx
