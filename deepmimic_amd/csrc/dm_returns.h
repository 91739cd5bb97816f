// TD(lambda) returns over a device-resident rollout: the critic targets of the reference's learner (learning/rl_util.py:3-18 compute_return under the end-of-path
// rules of learning/ppo_agent.py:251-284) for records that never leave HBM.  Included at the end of dm_host.cpp (shares its runtime shim); needs no env context.
//
// Layout: every array is time-major, row t = the N envs' values of control step t -- the way a sampler stacks the outputs of TorchVecEnv.  values[t] is the critic on the
// observation the action of step t was taken from, values[T] the critic on the observation after the last step; term_values[t] the critic on the terminal observation
// of step t (dm_set_terminal_outputs), used only where done[t] is set.  Per env column, backwards in time, with v_next the value behind step t:
//     not done: values[t + 1] | done, terminate Fail: val_fail | done, Succ: val_succ | done, Null (episode timer, clip end): term_values[t]
//     a step that closes a path (done[t], or t = T - 1):   ret[t] = r[t] + gamma * v_next
//     any other step:                                      ret[t] = r[t] + gamma * ((1 - lambda) * v_next + lambda * ret[t + 1])
// in fp64 from the fp32 inputs, the reference's association, no contraction, one rounding to fp32 at the store.  mask[t] = 0 for the steps of an episode that
// ended with valid == 0 inside the window (back to the previous done or to t = 0: the reference's driver discards such an episode), 1 elsewhere.
// ONE DEVIATION from the reference, which stores whole paths only: a rollout window cut at T is bootstrapped from values[T] like a Null path end, and a path
// that began before the window starts at row 0.
//
// One lane per env column: a row's loads are coalesced across the lanes of a wave, the per-lane chain is three dependent fp64 operations per step, and the six
// loads of row t - 1 are requested before row t's chain runs.  T x N x 32 bytes of traffic in all; latency-bound at rollout sizes (T = 32, N = 4096: 4 MB).
#pragma once

namespace dmr {

struct Row { float r, v, tv; int term, done, valid; };      // of step t: reward, values[t + 1], term_values[t], flags

struct Args {
    int T, N;
    const float *rewards, *values, *term_values; const int *terminate, *done, *valid;
    double gamma, lambda, val_fail, val_succ;
    float* returns; int* mask;
};

DM_HD Row load_row(const Args& a, int t, int n) {
    const size_t i = (size_t)t * a.N + n;
    Row w;
    w.r = a.rewards[i]; w.v = a.values[i + a.N]; w.tv = a.term_values[i]; w.term = a.terminate[i]; w.done = a.done[i];
    w.valid = a.valid ? a.valid[i] : 1;
    return w;
}
// the two expressions of learning/rl_util.py:9, 15: they must round like numpy's float64 arithmetic (no FMA)
DM_HD double path_end_return(double r, double gamma, double v_next) {
#pragma clang fp contract(off)
    double ret = r + gamma * v_next;
    return ret;
}
DM_HD double td_return(double r, double gamma, double lambda, double v_next, double next_ret) {
#pragma clang fp contract(off)
    double ret = r + gamma * ((1.0 - lambda) * v_next + lambda * next_ret);
    return ret;
}

__global__ void __launch_bounds__(64) k_td_lambda(Args a) {
    const int n = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (n >= a.N) return;
    double next_ret = 0;
    bool invalid = false;                 // the episode the scan is inside ended invalid
    Row cur = load_row(a, a.T - 1, n);
    for (int t = a.T - 1; t >= 0; --t) {
        Row prev = cur;
        if (t > 0) prev = load_row(a, t - 1, n);          // in flight while this row's chain runs
        const bool done = cur.done != 0;
        double v_next = (double)cur.v;
        if (done) v_next = (cur.term == TERM_FAIL) ? a.val_fail : (cur.term == TERM_SUCC) ? a.val_succ : (double)cur.tv;
        const double ret = (done || t == a.T - 1) ? path_end_return((double)cur.r, a.gamma, v_next) : td_return((double)cur.r, a.gamma, a.lambda, v_next, next_ret);
        if (done) invalid = cur.valid == 0;
        const size_t i = (size_t)t * a.N + n;
        a.returns[i] = (float)ret;
        if (a.mask) a.mask[i] = invalid ? 0 : 1;
        next_ret = ret;
        cur = prev;
    }
}

}  // namespace dmr

extern "C" {

int dm_td_lambda_returns(int device_id, int T, int N, const float* rewards_dev, const float* values_dev, const float* term_values_dev, const int32_t* terminate_dev,
                         const int32_t* done_dev, const int32_t* valid_dev, double gamma, double td_lambda, double val_fail, double val_succ,
                         float* returns_dev, int32_t* mask_dev, void* hip_stream) {
    if (T < 1 || N < 1) return fail("dm_td_lambda_returns: T and N must be >= 1");
    if (!rewards_dev || !values_dev || !term_values_dev || !terminate_dev || !done_dev || !returns_dev) return fail("dm_td_lambda_returns: null argument (only valid_dev and mask_dev may be NULL)");
    if ((long long)(T + 1) * N > 0x7fffffffLL) return fail("dm_td_lambda_returns: too many elements for one call");
    if (valid_device("dm_td_lambda_returns", device_id)) return -1;
    DevGuard guard(device_id);
    dmr::Args a;
    a.T = T; a.N = N; a.rewards = rewards_dev; a.values = values_dev; a.term_values = term_values_dev; a.terminate = terminate_dev; a.done = done_dev; a.valid = valid_dev;
    a.gamma = gamma; a.lambda = td_lambda; a.val_fail = val_fail; a.val_succ = val_succ; a.returns = returns_dev; a.mask = mask_dev;
    RT_LAUNCH(dmr::k_td_lambda, (N + 63) / 64, (rt_stream)hip_stream, a);
    return launch_status(0);
}

}  // extern "C"
