// Error string + version of libvlnce_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "common_opts.h"

static thread_local char g_err[512] = "";

void vlnce_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* vlnce_last_error(void) { return g_err; }
// major*100 + minor; 1.x: round-1 ABI (centered normalisation vectors, dual-input prologue,
// backward / data-path / returns entry points).  Struct layouts only ever grow at the end.
// 134: vlnce_set_option / vlnce_get_option (the library no longer reads environment variables).
// 136: vlnce_epilogue.bn (train-mode BatchNorm column sums added by the convolution) +
// vlnce_bn_finalize_sums.
// 137: vlnce_stem7_fwd.
// 138: vlnce_action_head_fwd / _bwd.
// 139: vlnce_attn_fwd_shared / _bwd_shared, vlnce_segment_sum.
// 140: option "m3" (conv_m3_kernel).
// 141: vlnce_rnn_seq_fwd2 / _bwd2 / _wgrad, vlnce_linear_rows_fwd / _bwd, vlnce_ppo_loss, vlnce_prologue.options (per-launch dispatch options).
// 142: plane format 2 (fp16 planes, three plane products per multiply): vlnce_prologue.w_format, a
// `format` argument of vlnce_conv2d_split_weights / _pack_weights, `w_format` of vlnce_stem7_fwd;
// option "conv_math" defaults to 2.
// 143: vlnce_bn_bwd takes a workspace (vlnce_bn_bwd_workspace_floats): partial sums instead of atomics;
// vlnce_conv2d_prepare_weights / vlnce_weight_job (all weight images of a trainable trunk in one launch).
// 144: vlnce_lstm_rollout_supported / _workspace_bytes / _fwd / _bwd (the LSTM state-encoder rollout in one launch per direction).
// 145: vlnce_conv2d_wgrad_last_path (which weight-gradient kernel the thread's last vlnce_conv2d_wgrad ran on).
// vlnce_gn_bwd_workspace_floats grows: the [N,groups,2] segment is padded to 16 bytes, and [N,C,2] per-sample
// shares of dgamma / dbeta are added up in sample order (no atomics).
// 146: vlnce_conv2d_last_kernel / vlnce_conv2d_wgrad_last_kernel (which kernel INSTANCE the thread's last
// launch ran on: family, plane format, tile / mode / template arguments; VLNCE_CONV_KERNEL_*).
// 147: vlnce_traj_append / vlnce_traj_sensor, vlnce_dagger_mix_actions (DAgger rollout collection on the device).
// 148: vlnce_epilogue.stats_only (a convolution that takes its BatchNorm statistics and stores no output),
// vlnce_prologue.regen (a block end that computes conv3's output again instead of reading it), options "r3", "s3_wgs".
// 149: vlnce_il_loss / vlnce_il_loss_supported, vlnce_pair_mse (the imitation-learning objective and the progress
// monitor's term, each one launch with its gradient).
// 150: vlnce_gemm_last_kernel (which igemm_kernel instance the thread's last vlnce_gemm launched: loader pair,
// tile, split-K factor, zero-fill, second pass; VLNCE_GEMM_KERNEL).  vlnce_gemm refuses a scale / shift that
// is not 16-byte aligned, and refuses every bad argument before it launches anything.
// 151: vlnce_waypoint_eval / _bwd / _supported, vlnce_wp_part (WaypointPolicy.evaluate_actions' distribution
// arithmetic: one launch forward, one backward, no host synchronisation); option "waypoint_dist".
// 152: vlnce_grad_sumsq / vlnce_adam_step / vlnce_adam_supported / _max_tensors / _chunk (clip_grad_norm_ + Adam
// over a list of tensors in two launches; csrc/optim.hip).
// 153: vlnce_rollout_copy / _copy_supported / _gather, vlnce_ppo_advantages (the DD-PPO rollout storage's insert,
// after_update, minibatch gather and advantages, one launch each; csrc/rollout.hip).
// 154: vlnce_waypoint_act / _act_supported, vlnce_waypoint_history_pick (WaypointPolicy.act behind the net in one launch,
// the trainer's observation-history pick in one more; csrc/waypoint_act.hip); option "waypoint_act".
// 155: vlnce_waypoint_feature_pick / _feature_rows (the trunk-feature cache of the Waypoint DD-PPO loop: the
// history features of the next step and the [B, P + 1, F] encoder batch, one launch each;
// csrc/waypoint_features.hip).
extern "C" int vlnce_version(void) { return 155; }

// ---- dispatch options: one int per name, process-wide, relaxed atomics (a tuning / test knob,
// not a synchronisation point: set them before the launches they are meant for)
namespace {
struct OptDef {
  const char* name;
  int def;
};
const OptDef kOpts[VLNCE_OPT_COUNT] = {
    {"conv_math", 2},   {"p3", 2},          {"p3_tile", 0},         {"s3", 1},
    {"u3", 1},          {"u3_waves", 8},    {"x3_tile", 0},         {"igemm_tile", 0},
    {"igemm_nobuf", 0}, {"igemm_no_splitk", 0}, {"wgrad_tile", 64}, {"rollout_one_xcd", 0},
    {"m3", 1},          {"r3", 1},          {"s3_wgs", 0},          {"waypoint_dist", 0},
    {"waypoint_act", 0},
};
std::atomic<int> g_opt[VLNCE_OPT_COUNT] = {
    {2}, {2}, {0}, {1}, {1}, {8}, {0}, {0}, {0}, {0}, {64}, {0}, {1}, {1}, {0}, {0}, {0},
};
int opt_index(const char* name) {
  if (name)
    for (int i = 0; i < VLNCE_OPT_COUNT; ++i)
      if (strcmp(name, kOpts[i].name) == 0) return i;
  return -1;
}
}  // namespace

namespace {
thread_local const int* t_call_opts = nullptr;   // vlnce_prologue.options of the launch being dispatched
}
VlnceOptScope::VlnceOptScope(const int* per_call) : prev(t_call_opts) { t_call_opts = per_call; }
VlnceOptScope::~VlnceOptScope() { t_call_opts = prev; }

int vlnce_opt(int id) {
  if (t_call_opts && t_call_opts[id] >= 0) return t_call_opts[id];
  return g_opt[id].load(std::memory_order_relaxed);
}

extern "C" int vlnce_option_count(void) { return VLNCE_OPT_COUNT; }

extern "C" int vlnce_option_index(const char* name) { return opt_index(name); }

extern "C" int vlnce_set_option(const char* name, int value) {
  const int i = opt_index(name);
  if (i < 0) {
    vlnce_set_error("vlnce_set_option: unknown option '%s'", name ? name : "(null)");
    return 1;
  }
  g_opt[i].store(value, std::memory_order_relaxed);
  return 0;
}

extern "C" int vlnce_get_option(const char* name, int* value) {
  const int i = opt_index(name);
  if (i < 0 || !value) {
    vlnce_set_error("vlnce_get_option: unknown option '%s'", name ? name : "(null)");
    return 1;
  }
  *value = g_opt[i].load(std::memory_order_relaxed);
  return 0;
}

extern "C" int vlnce_option_default(const char* name, int* value) {
  const int i = opt_index(name);
  if (i < 0 || !value) {
    vlnce_set_error("vlnce_option_default: unknown option '%s'", name ? name : "(null)");
    return 1;
  }
  *value = kOpts[i].def;
  return 0;
}
