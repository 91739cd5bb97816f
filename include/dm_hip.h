/* dm_hip.h -- C-ABI of the MI355X-native DeepMimic imitate environment (libdm_hip.so).
 *
 * This is the drop-in boundary for the reference's SWIG class `cDeepMimicCore`
 * (/root/reference/DeepMimicCore/DeepMimicCore.h:9-119, exported by DeepMimicCore.i:1-34) restricted to
 * the `--scene imitate` hot path.  One `dm_ctx` owns N independent envs (N = 1 reproduces one
 * cDeepMimicCore instance) on one GPU and one HIP stream.  Plain pointers and sizes only; every function
 * returns 0 on success and a negative code on error, `dm_last_error()` gives the message.  The library
 * never aborts the caller (the reference asserts: DeepMimicCore.cpp:36-40, scenes/SceneBuilder.cpp:60-64).
 *
 * Array arguments are HOST pointers unless the name ends in `_dev` / the flag DM_DEVICE_PTRS is given.
 */
#ifndef DM_HIP_H
#define DM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Layout version of this header: bumped whenever dm_create_info / dm_scene_tables gain fields or an entry point changes meaning.  A host checks
 * `dm_abi_version() == DM_ABI_VERSION` (and a binding that mirrors the structs by hand, `dm_struct_sizes`) once after loading the library: the
 * tables are read as the CURRENT layout, a caller built against an older header would hand over a shorter struct. */
#define DM_ABI_VERSION 5

typedef struct dm_ctx dm_ctx;

typedef struct {
    int num_envs;            /* N independent characters */
    int device_id;           /* HIP device ordinal */
    uint64_t seed;           /* cDeepMimicCore::SeedRand (DeepMimicCore.cpp:20-23); keys the per-env reset RNG */
    int precision;           /* 32 (default, production) or 64 (algorithm-parity build of the same kernels) */
    int max_contacts;        /* manifold cap per character, <= 20 (0 -> 20) */
    int env_id_offset;       /* global id of env 0 (multi-GPU shards keep global RNG streams) */
    int wave_packing;        /* characters per wavefront of the step kernel: 0 = default (2 where possible; env DM_DUO=0 -> 1), 1, or
                                2 (biped class, even num_envs; same results up to fp rounding, dm_device_duo.h) */
    int physics;             /* rigid-body step: 0 / 1 = DM-physics v1 (default: analytic contact set rebuilt every substep, the nearer
                                row of a revolute limit), 2 = v2 (Bullet's manifold semantics as recalled, SURVEY App. C items 4, 7:
                                both rows of every revolute limit; one persistent manifold per link against the ground, refreshed and
                                given ONE new support point per substep, <= 4 points, breaking threshold 0.02 x angular-motion disc).
                                v2 has its own instantiations of the kernels (AMP code + manifolds), one or -- biped class, since round 4 -- two
                                characters per wavefront; not with the dribble ball; DESIGN.md 4.6 */
} dm_create_info;

/* Raw scene tables in the reference's in-memory layout (all host pointers, copied at create time). */
typedef struct {
    int num_joints;
    const double* joint_mat;     /* J x 19  cKinTree::tJointDesc rows   (anim/KinTree.h:24-47)  */
    const double* body_defs;     /* J x 17  cKinTree::tBodyDef rows     (anim/KinTree.h:49-70)  */
    const double* pd_params;     /* J x 2   Kp, Kd                      (sim/PDController.cpp:50-93) */
    int num_frames;
    const double* frames;        /* F x (1+P) duration + pose           (anim/Motion.cpp:344-378) */
    int loop;                    /* "Loop": "wrap"                      (anim/Motion.cpp:302-320) */
    const int32_t* fall_mask;    /* J  fall-contact links               (scenes/SceneSimChar.cpp:460-476) */
    /* arg-file keys */
    int num_sim_substeps;        /* --num_sim_substeps */
    double world_scale;          /* --world_scale (only scales Bullet's absolute tolerances) */
    double gravity[3];           /* --gravity, default (0,-9.8,0) */
    int sync_char_root_pos, sync_char_root_rot, enable_fall_end, enable_char_contact_fall;
    int enable_root_rot_fail, enable_rand_char_placement, enable_rand_rot_reset;
    double time_lim_min, time_lim_max;   /* episode timer, uniform (util/Timer.cpp:55-73); inf = no limit */
    /* controller file keys (sim/CtController.cpp:161-172) */
    int enable_phase_input, record_world_root_pos, record_world_root_rot;
    double query_rate;
    /* DM-physics v1 constants; 0 selects the default */
    double friction, erp; int solver_iters;
    int disable_self_collision;  /* 0 (default): links of the character collide with each other except parent-child pairs, as
                                    btMultiBody's default m_hasSelfCollision does (sim/SimCharacter.cpp:857,873,919) */
    /* `--scene imitate_amp` (scenes/SceneImitateAMP.cpp): CalcReward = 0, CheckTerminate = fall only, AMP observations on */
    int scene_amp;
    int enable_amp_obs_local_root;   /* --enable_amp_obs_local_root (SceneImitateAMP.cpp:30,42) */
    /* ---- goal-conditioned AMP task scenes, scene_amp must be set:
     * 1 = `--scene target_amp` (scenes/SceneTargetAMP.cpp), 2 = `--scene heading_amp` (scenes/SceneHeadingAMP.cpp).  RecordGoal has
     * size 3, CalcReward is the task reward, CheckTerminate adds the target-distance failure; keys of ParseArgs (:92-106 / :55-84) */
    int scene_goal;
    double rand_target_time_min, rand_target_time_max, max_target_dist, target_succ_dist, tar_fail_dist, tar_speed;
    int enable_min_tar_vel;
    double pos_reward_scale, max_heading_turn_rate, sharp_turn_prob, speed_change_prob, tar_speed_min, tar_speed_max, vel_reward_scale;
    /* ---- multi-clip dataset (`--kin_ctrl clips`, anim/ClipsController.cpp): `frames` is the concatenation of the clips, clip c owns
     * rows clip_starts[c] .. clip_starts[c+1]-1; a reset draws the clip by weight (SelectNewMotion, :226-243).  0 = single clip. */
    int num_clips;
    const int32_t* clip_starts;   /* num_clips + 1 */
    const double* clip_weights;   /* num_clips */
    const int32_t* clip_loops;    /* num_clips */
    /* ---- scene_goal 3 = `--scene heading_amp_getup` (scenes/SceneHeadingAMPGetup.cpp): heading_amp + a get-up timer -- RecordGoal has
     * size 4 (+ get-up phase, :123-130), the get-up reward while it runs (:4-38), no contact fall while it runs (:255-264), in test mode
     * a fall starts it (:244-253), in train mode a failed episode continues as a recovery episode with probability
     * recover_episode_prob (:109-121, 40-56).  getup_time = duration of the longest get-up clip (CalcGetupTime :266-291);
     * getup_clip_mask: bit c set = clip c is a get-up motion (--getup_motion_ids).
     * scene_goal 4 = `--scene strike_amp` (scenes/SceneStrikeAMP.cpp): target_amp with a target point in the air, RecordGoal size 4
     * (target in the origin frame + hit phase, :414-434), near / far / hit reward (:23-187), success and target-contact termination
     * (:485-541); strike_mask / fail_tar_mask: bit j = link j (--strike_bodies / --fail_tar_contact_bodies). */
    int mode_test;                /* 1 = cRLScene::eModeTest at creation; dm_set_mode changes it */
    double getup_time, getup_height_root, getup_height_head, recover_episode_prob;
    int head_id, getup_clip_mask;
    double tar_near_dist, tar_far_prob, target_radius, target_hit_reset_time, init_hit_prob, hit_tar_speed, tar_reward_scale;
    double target_min[3], target_max[3];
    int strike_mask, fail_tar_mask;
    /* ---- scene_goal 5 = `--scene dribble_amp` (scenes/SceneDribbleAMP.cpp): target_amp with a ball -- a free rigid sphere in the world
     * (BuildTarObjs :398-420: radius, mass 0.43, friction 0.4, linear / angular damping 0.4) the character has to move to the target.
     * RecordState gains 15 entries (the ball in the origin frame, :554-590), RecordGoal is the direction / distance from the ball to the
     * target (:276-302), the reward :21-106, success / distance termination :343-379, 454-475.  One character per wavefront.
     * ball_friction is the combined coefficient of a ball contact (ball 0.4 x link / ground 0.9). */
    double rand_tar_obj_time_min, rand_tar_obj_time_max, min_tar_obj_dist, max_tar_obj_dist;
    double ball_radius, ball_mass, ball_friction, ball_lin_damping, ball_ang_damping;
    /* ---- random perturbations (`--enable_rand_perturbs`, scenes/SceneSimChar.cpp:41-51, 92-99, 205-256, 618-626, 952-956; sim/Perturb.cpp;
     * sim/PerturbManager.cpp; sim/World.cpp:93-96): every U[perturb_time_min, perturb_time_max] seconds a force of U[min_perturb,
     * max_perturb] N in a uniformly drawn direction acts at the centre of mass of a random body part for U[min, max duration] seconds
     * (`min_pertrub_duration` [sic] / `max_perturb_duration`).  perturb_part_mask: bit j = part j may be hit (--perturb_part_ids), 0 = any.
     * Cleared and re-armed by every scene reset.  Needs 2 * perturb_time_min >= max_perturb_duration (two forces at once at most).
     * perturb_time_min = perturb_time_max = +infinity is accepted and means "the rows exist, nothing fires by itself": the context carries the per-env
     * perturbation rows and runs the kernels that apply them, every reset makes its one draw, and no force is ever drawn -- the rows then serve dm_push_where
     * alone (the other ranges may be 0). */
    int enable_rand_perturbs;
    double perturb_time_min, perturb_time_max, min_perturb, max_perturb, min_perturb_duration, max_perturb_duration;
    int perturb_part_mask;
} dm_scene_tables;

/* DM_END_EPISODE_EARLY: an env whose episode is over after update u of the call (fall contact, clip end, episode timer) takes no
 * further updates in this call -- the reference's driver checks IsEpisodeEnd after EVERY Update and ends the episode there
 * (DeepMimic.py:62-80), so the terminal reward / state are those of that moment, not of the next action boundary. */
enum { DM_DEVICE_PTRS = 1, DM_AUTO_RESET = 2, DM_OPEN_LOOP = 4, DM_NO_EMIT = 8, DM_END_EPISODE_EARLY = 16 };

const char* dm_last_error(void);
/* 0 for libdm_hip.so; 1 for the CPU fiber-emulator build of the same sources (tests/emu, test infrastructure) */
int dm_is_emulator(void);
/* DM_ABI_VERSION the library was built with; out[0] = sizeof(dm_create_info), out[1] = sizeof(dm_scene_tables) as the library sees them */
int dm_abi_version(void);
int dm_struct_sizes(int32_t* out);

/* cDeepMimicCore ctor + ParseArgs + Init  (DeepMimicCore.cpp:9-54) */
int dm_create(const dm_create_info* info, const dm_scene_tables* tables, dm_ctx** out);
int dm_destroy(dm_ctx* ctx);
/* GetStateSize / GetGoalSize / GetActionSize (+ pose, links, dofs, frames of clip 0): out[8] = S,G,A,P,J,D,F,N */
int dm_dims(const dm_ctx* ctx, int32_t* out);
/* out[0] = physics version the ctx runs (1 or 2), out[1] = effective contact cap per character (physics 2: min(max_contacts, (64 - 2 x limited joints) / 3)) */
int dm_physics_info(const dm_ctx* ctx, int32_t* out);
double dm_motion_duration(const dm_ctx* ctx);
/* Run the kernels of this ctx on an external HIP stream (e.g. torch's current stream); NULL restores the own (non-blocking) stream.
 * The legacy default stream has the NULL handle too: dm_set_stream_default selects IT (torch's default stream when no torch.cuda.Stream is
 * current), so that work enqueued by the caller on the default stream and this ctx's launches are ordered against each other. */
int dm_set_stream(dm_ctx* ctx, void* hip_stream);
int dm_set_stream_default(dm_ctx* ctx);
/* The HIP stream handles of the ctx: *out_own = the non-blocking stream dm_create made for it, *out_current = the stream its kernels are
 * launched on right now (own stream, an external one, or NULL = the legacy default stream).  Either pointer may be NULL.  For callers that
 * order other work against the ctx with events (torch.cuda.ExternalStream(own), hipStreamWaitEvent): env groups on their own streams whose
 * records feed one collective (bench.py, deepmimic_amd/groups.py). */
int dm_get_stream(const dm_ctx* ctx, void** out_own, void** out_current);
int dm_synchronize(dm_ctx* ctx);

/* cDeepMimicCore::SetMode (DeepMimicCore.cpp:472-479 -> cRLSceneSimChar::SetMode / ResetTimers, scenes/RLSceneSimChar.cpp:
 * 270-290): the episode-timer range drawn at the next resets; train = (time_lim_min, time_lim_max), test = time_end_lim_*. */
int dm_set_time_limits(dm_ctx* ctx, double time_lim_min, double time_lim_max);
/* `--timer_type exp --time_lim_exp E` (scenes/Scene.cpp:19-23, util/Timer.cpp:27-45, 64-67): every reset -- explicit or inside a DM_AUTO_RESET
 * launch -- then draws min(time_lim_min + Exp(mean E), time_lim_max) instead of U[time_lim_min, time_lim_max].  0 (the default) = uniform timer.
 * Annealing blends E like the limits (cTimer::tParams::Blend): call again with the blended value. */
int dm_set_timer_exp(dm_ctx* ctx, double time_lim_exp);

/* cDeepMimicCore::Reset (DeepMimicCore.cpp:61-65).  env_ids NULL -> all envs.  kin_times / max_times NULL ->
 * per-env counter-based RNG: kin time ~ U[0,duration) (scenes/SceneImitate.cpp:494-500), timer ~ U[min,max]. */
int dm_reset(dm_ctx* ctx, const int32_t* env_ids, int n, const double* kin_times, const double* max_times);
/* cDeepMimicCore::SetAction for every env (DeepMimicCore.cpp:221-230): actions N x A float32 */
int dm_set_action(dm_ctx* ctx, const float* actions, int flags);
/* cDeepMimicCore::Update(timestep) n_updates times for every env (DeepMimicCore.cpp:56-59) */
int dm_update(dm_ctx* ctx, double timestep, int n_updates);
/* RecordState / CalcReward / CheckTerminate / CheckValidEpisode / IsEpisodeEnd / NeedNewAction for every env
 * (DeepMimicCore.cpp:191-204,450-458,...); any output may be NULL */
int dm_query(dm_ctx* ctx, float* states, float* rewards, int32_t* terminate, int32_t* valid, int32_t* episode_end,
             int32_t* need_new_action, int flags);
/* Batched control step = [SetAction] + n_updates x Update + query (+ auto reset), one kernel launch.
 * actions may be NULL (keep the latched targets).  With DM_AUTO_RESET, envs whose episode ended are reset after
 * their terminal reward/flags are written and `states` holds the first observation of the new episode (the observation of the moment
 * the episode ended goes to the buffers of dm_set_terminal_outputs, when bound). */
int dm_step_batch(dm_ctx* ctx, const float* actions, double timestep, int n_updates, float* states, float* rewards,
                  int32_t* terminate, int32_t* valid, int32_t* episode_end, int flags);
/* Hand back the observation of the moment an episode ended.  Binds two DEVICE buffers to the ctx: term_states_dev N x S floats, term_goals_dev
 * N x dm_goal_size() floats (goal scenes; may be NULL); NULL, NULL unbinds.  While they are bound, every launch with DM_AUTO_RESET that emits (dm_step_batch,
 * dm_step_batch_amp with a non-NULL `states`, and the loop of dm_bench_rollout) writes, for each env it resets -- episode_end != 0 or valid == 0 -- the RecordState row
 * and the RecordGoal row the env had when its episode ended (with DM_END_EPISODE_EARLY: at the update that ended it), i.e. what `states` / the goals held
 * before the reset overwrote them with the first observation of the next episode: the path-end state of learning/path.py:12-22 that the critic
 * bootstraps a timer end from (learning/ppo_agent.py:251-266).  Rows of envs the launch did not reset are NOT written; an invalid episode's row is
 * written as computed, non-finite values included.  Everything else the launch writes, and the stored env state, is bit for bit what it is with
 * nothing bound; without DM_AUTO_RESET the binding has no effect.  dm_step_envs (the subset route) ignores the binding.  The buffers must stay
 * allocated while bound; the rows are written on the ctx stream by the step kernel itself. */
int dm_set_terminal_outputs(dm_ctx* ctx, float* term_states_dev, float* term_goals_dev);

/* dm_step_batch for a SUBSET of the ctx's envs: env_ids[n] distinct ids; actions (n x A, NULL = keep the latched targets), states (n x S), rewards,
 * flags, amp_obs (n x dm_amp_obs_size(), imitate_amp scenes) and clocks (n x 5 doubles: kin_time, ctrl_time, init_time_offset, timer_time, timer_max
 * after the call) are COMPACT host arrays, row i <-> env_ids[i]; any output may be NULL.  The other envs are not touched.  One character per
 * wavefront (the kernel of an odd-sized / one-env ctx: an env stepped here follows the trajectory it would follow alone in a ctx of its own).  This is
 * what a process that owns the GPU for several one-env callers runs when some of them have asked for their next control step and others have not
 * (deepmimic_amd/broker.py: W cDeepMimicCore workers -- the reference's `mpiexec -n W`, mpi_run.py:16-24 -- behind ONE launch per control step). */
int dm_step_envs(dm_ctx* ctx, const int32_t* env_ids, int n, const float* actions, double timestep, int n_updates, float* states, float* rewards,
                 int32_t* terminate, int32_t* valid, int32_t* episode_end, float* amp_obs, double* clocks, int flags);

/* ---- `--scene imitate_amp` only (dm_scene_tables.scene_amp): adversarial-motion-prior observations
 * GetAMPObsSize (scenes/SceneImitateAMP.cpp:76-86): 2 x (pose features + velocity features); 0 for a plain imitate scene */
int dm_amp_obs_size(const dm_ctx* ctx);
/* RecordAMPObsAgent for every env (:101-113): [pose_t, pose_t-1, vel_t, vel_t-1] of the simulated character, t-1 = the
 * state at the last action latch (cSceneImitateAMP::UpdateHist, :166-171).  amp_obs N x dm_amp_obs_size() float32. */
int dm_query_amp(dm_ctx* ctx, float* amp_obs, int flags);
/* dm_step_batch that also writes RecordAMPObsAgent at the end of the control step (before any auto reset, i.e. the
 * end-of-path observation of a finished episode, learning/amp_agent.py:239-242). */
int dm_step_batch_amp(dm_ctx* ctx, const float* actions, double timestep, int n_updates, float* states, float* rewards,
                      int32_t* terminate, int32_t* valid, int32_t* episode_end, float* amp_obs, int flags);
/* RecordAMPObsExpert (:115-138), n samples: clip frames at times[i] and one control period earlier (raw cMotion::CalcFrame /
 * CalcFrameVel).  times NULL -> drawn ~ U[0, duration) from the ctx's counter-based generator (the reference draws from the
 * scene RNG); ground_h NULL -> 0 (the reference passes the kin character's origin height).  out n x dm_amp_obs_size(). */
int dm_amp_expert(dm_ctx* ctx, int n, const double* times, const double* ground_h, float* out, int flags);
/* Multi-clip variant (SampleExpertMotion, SceneImitateAMP.cpp:115-138 with a cClipsController): clips[i] = dataset clip of sample i;
 * clips NULL -> drawn by weight (and times ~ U[0, that clip's duration)) from the ctx generator.  Host pointers. */
int dm_amp_expert_clips(dm_ctx* ctx, int n, const int32_t* clips, const double* times, const double* ground_h, float* out);
/* The same draws made ON THE DEVICE: n expert observations whose clip ids and sample times a small kernel (k_amp_expert_draw) writes into scratch the context owns
 * (grown on demand by doubling; only a call that grows it allocates, which waits for the device, and no block -- the outgrown ones included -- is freed before dm_destroy:
 * after one call with a very large n, 12 bytes per sample of the largest n, at most twice that with the outgrown blocks, stay with the context), consumed by the launch
 * behind dm_amp_expert_clips.  Every pointer is a device pointer; asynchronous on
 * the context's current stream, no host read, no synchronisation.  Sample i draws exactly what the host routes draw with their counter at `call`:
 *   clip: u = rand01(seed, env_id_offset + 0x434C50, call, i) searched in the clip cdf (dm_clip_table); time: clip duration * rand01(seed, env_id_offset + 0x414D50, call, i);
 *   a single-clip scene draws no clip and its time is the motion's duration * rand01(seed, env_id_offset + 0x414D50, call, i)     (dm_amp_expert with times NULL).
 * `call` is the CALLER's counter: the context's own counter is neither read nor advanced.  ground_h_dev NULL -> 0.  clips_out_dev int32[n] / times_out_dev double[n]
 * (either may be NULL) receive the draws.  out_dev n x dm_amp_obs_size().  Refused: a context without AMP observations, n < 1, out_dev NULL. */
int dm_amp_expert_draw(dm_ctx* ctx, int n, uint64_t call, const double* ground_h_dev /* NULL: 0 */, float* out_dev, int32_t* clips_out_dev /* may be NULL */,
                       double* times_out_dev /* may be NULL */);

/* ---- goal scenes (dm_scene_tables.scene_goal != 0)
 * RecordGoal for every env (SceneTargetAMP.cpp:195-223 / SceneHeadingAMP.cpp:150-166 / SceneHeadingAMPGetup.cpp:123-130 /
 * SceneStrikeAMP.cpp:414-434): goals N x dm_goal_size() float32 */
int dm_goal_size(const dm_ctx* ctx);          /* GetGoalSize: 0 (no goal scene), 3, or 4 (heading_amp_getup, strike_amp) */
int dm_query_goal(dm_ctx* ctx, float* goals, int flags);
/* the goals written by the most recent dm_step_batch / dm_query (no launch): what the agent reads next to `states` */
int dm_last_goals(dm_ctx* ctx, float* goals);
/* RecordGoal of the last emit into a DEVICE buffer (N x goal size floats), asynchronously on the ctx stream: no host round trip */
int dm_last_goals_device(dm_ctx* ctx, float* goals_dev);
/* Goal state snapshot (tests, checkpointing): N x 12 doubles = target pos(3), target heading, target speed, target timer time,
 * target timer max, COM at the last action(3), controller time of the last action, draws consumed so far.  NULL = leave as is. */
int dm_get_goal_state(dm_ctx* ctx, double* out);
int dm_set_goal_state(dm_ctx* ctx, const double* in);
/* the scene-specific part of the goal state, N x 8 doubles: [0..1] heading_amp_getup {get-up timer time, unused}; strike_amp {target hit
 * (0 / 1), scene time of the hit (-1 = none)}; [2..6] dribble_amp {ball position at the last action (3), target-object timer time, limit};
 * [7] reserved: reads 0, is ignored on write (the goal row's next slot is the env's own draw key, dm_set_env_keys, which a restored aux block never re-keys) */
int dm_get_goal_aux(dm_ctx* ctx, double* out);
int dm_set_goal_aux(dm_ctx* ctx, const double* in);
/* the random-perturbation state (enable_rand_perturbs), N x 16 doubles per env: [0] time since the last perturbation, [1] time of the next one
 * (cSceneSimChar::tPerturbParams::mTimer / mNextTime), [2] draw counter, then two force slots of 6: {body part + 1 (0 = free), force x, y, z,
 * duration, elapsed} (tPerturb, sim/Perturb.h), [15] unused.  For checkpointing and for tests that place a known force. */
int dm_get_perturb_state(dm_ctx* ctx, double* out);
int dm_set_perturb_state(dm_ctx* ctx, const double* in);
/* cRLScene::SetMode (DeepMimicCore.cpp SetMode -> scene): 0 train, 1 test.  Only the goal scenes read it on the device (get-up on a
 * fall instead of termination, recovery episodes, strike_amp's test reward); the episode-timer limits of the two modes are the
 * caller's business (dm_set_time_limits). */
int dm_set_mode(dm_ctx* ctx, int test_mode);
/* Give the listed envs a draw key of their own: env_ids[i] becomes what env 0 of a fresh ONE-env context created with seed seeds[i] (< 2^53) is before its first
 * reset -- every counter-based draw it makes from then on (clip, clip time, yaw, episode limit, goal re-sampling, perturbations) is keyed (seeds[i], env 0), its draw
 * and episode counters start at 0, its DM-physics v2 manifolds are empty -- so that W one-env callers can share one context and one launch per control step and
 * still see the trajectories of W private contexts (the shared-owner facade, deepmimic_amd/broker.py; the reference's deployment is one cDeepMimicCore per MPI
 * worker, mpi_run.py:16-24).  Reset the envs next (dm_reset), as dm_create does.  Synchronises the ctx stream. */
int dm_set_env_keys(dm_ctx* ctx, const int32_t* env_ids, int n, const uint64_t* seeds);
/* durations[k], cdf[k] of the num_clips clips of a `--kin_ctrl clips` dataset (cClipsController::mClipsCDF, anim/ClipsController.cpp; one entry -- the clip's
 * duration, 1 -- for a single-clip scene): what dm_amp_expert_clips draws its clips and clip times from */
int dm_clip_table(const dm_ctx* ctx, double* durations, double* cdf);
/* dribble_amp: the ball of every env, N x 13 doubles = position(3), rotation w x y z (4), linear velocity(3), angular velocity(3)
 * (cSimObj::GetPos / GetRotation / GetLinearVelocity / GetAngularVelocity of the target object) */
int dm_get_obj_state(dm_ctx* ctx, double* out);
int dm_set_obj_state(dm_ctx* ctx, const double* in);
/* DM-physics v2 (dm_create_info.physics = 2): the persistent link-vs-ground manifolds, N x J x 25 doubles per link = {point count (0..4),
 * 4 x (the point on the link in body coordinates (3), the point on the plane x, z, distance)} -- device state that dm_get_state / dm_set_state do
 * not carry (dm_set_state(pose) EMPTIES them, as a fresh pose has no contact history).  A checkpoint or a rollback under v2 is
 * dm_get_state + dm_get_manifolds / dm_set_state THEN dm_set_manifolds.  Error when the ctx runs v1. */
int dm_get_manifolds(dm_ctx* ctx, double* out);
int dm_set_manifolds(dm_ctx* ctx, const double* in);
/* clip each env's kinematic character was reset to (multi-clip datasets), N int32 */
int dm_get_clips(dm_ctx* ctx, int32_t* out);
/* Set that bookkeeping (N int32): the clip the kinematic controller counts as active -- the reference draws the clip time of a reset over the duration of the
 * clip that was active BEFORE the reset (scenes/SceneImitate.cpp:331-335, 494-500), and cClipsController::Init already selected one at construction
 * (anim/ClipsController.cpp:24-34).  The character's state is not touched; only a reset through the draw tape reads it. */
int dm_set_clips(dm_ctx* ctx, const int32_t* clips);

/* BuildStateOffset/Scale, BuildActionOffset/Scale/BoundMin/BoundMax, BuildStateNormGroups (DeepMimicCore.cpp:232-448) */
int dm_build_offsets_scales(const dm_ctx* ctx, double* s_off, double* s_scale, double* a_off, double* a_scale,
                            double* a_min, double* a_max, int32_t* s_norm_groups);

/* Env state snapshot (parity tests, checkpointing): pose/vel N x P, kin N x 7 (origin pos + rot), clocks N x 5
 * (kin_time, ctrl_time, init_time_offset, timer_time, timer_max), tar N x P.  Any pointer may be NULL. */
int dm_get_state(dm_ctx* ctx, double* pose, double* vel, double* tar, double* kin, double* clocks, int32_t* flags);
int dm_set_state(dm_ctx* ctx, const double* pose, const double* vel, const double* tar, const double* kin,
                 const double* clocks, const int32_t* flags);

/* Component taps used by the parity tests (no reference analogue): what = 0 SPD torque, 1 one rigid-body
 * substep of length `dt` with the latched torque, 2 SPD-model mass matrix / bias force.
 * 5: one scene update of length `dt` (dm_update(dt, 1): no action, no outputs) on the tap instantiation of the
 * two-characters-per-wavefront kernel, which writes the "contacts", "rows" and "limit_rest" taps only -- the collision routine of that
 * kernel on its own; fails where no such family serves the context (dm_get_debug "family" reports the one that ran).
 * "limit_rest" (N x 4, counted over that one update): Gauss-Seidel sweep iterations that jumped over the resting joint-limit blocks |
 * that visited them because this env's own limit rows were not at rest | only because its partner's were not; sweeps in which
 * the decision changed between iterations.
 * After the call dm_get_debug copies the requested tap: name in {"H","C","vstar","lambda","rows","tau",
 * "kin_pose","kin_vel","reward_terms","links","contacts","limit_rest"}; out must hold the full N x ... array of doubles.
 * "contacts" (N x max_contacts x 8, max_contacts as dm_physics_info reports it): the contact slots of the last substep right
 * after collision detection, in slot order: point x (3), normal n (3), distance, link ids a | b << 8 (b = 255: the ground,
 * 254: the free body; a = 254: the free body on the ground).  The number of slots in use is "rows"[1]; the others read 0.
 * "tau" and "fallback" need no dm_probe.  "fallback" (N doubles): the number of rigid-body substeps the env has spent on
 * the 64-lane fallback of the two-characters-per-wavefront kernel (a pair of which one character had more than 32
 * constraint rows in that substep; both characters count it) since dm_create or the last dm_set_state -- a statistic
 * of the production kernels, kept in the pad word of the env's kin row; 0 on the one-character-per-wavefront kernels.
 * "borrowed" (N doubles): likewise the substeps in which ONE character of the pair had more than 32 rows, the two together
 * at most 64, and the pair stayed on the two-per-wavefront path with the heavy character's rows 32.. on lanes of its
 * partner's half (kept in the pad word of the env's clock row).
 * "family" (N doubles, all equal; needs no dm_probe): the kernel family -- its id in the table of deepmimic_amd/csrc/dm_families.h,
 * one compiled object per precision -- of the last step-kernel launch of the context (dm_step_*, dm_bench_rollout, the profiled
 * step of dm_probe 3 / 4); -1 before the first. */
int dm_probe(dm_ctx* ctx, int what, double dt);
int dm_set_tau(dm_ctx* ctx, const double* tau /* N x D, generalized-velocity layout */);
int dm_get_debug(dm_ctx* ctx, const char* name, double* out);

/* Fixed-action rollout timed with HIP events on the ctx stream: `steps` control steps of `n_updates` updates
 * after `warmup` untimed ones.  actions_dev NULL with DM_OPEN_LOOP tracks the clip.  Returns the elapsed GPU
 * milliseconds of the timed region in *elapsed_ms. */
int dm_bench_rollout(dm_ctx* ctx, int warmup, int steps, double timestep, int n_updates, int flags,
                     float* states_dev, float* rewards_dev, double* elapsed_ms);

/* ---- Multi-GPU: one process per GPU, env shards are independent; the only exchange is the all-gather of the
 * learner record {state[S], reward, terminate} once per control step, RCCL over xGMI.  For hosts that stay in C/C++ (the
 * reference's own launcher is `mpiexec -n W`, mpi_run.py:16-24); deepmimic_amd/dist.py is the torch.distributed mirror.
 * Bootstrap is the caller's: rank 0 calls dm_comm_unique_id, ships the 128 bytes to the other ranks by its own means (MPI_Bcast,
 * a file, a torch store) and every rank calls dm_comm_create (= ncclCommInitRank).  librccl is loaded lazily (dlopen) by these
 * calls only; world == 1 with a NULL unique id needs no RCCL at all (the gather is a device copy). */
typedef struct dm_comm dm_comm;
int dm_comm_unique_id(void* out_128_bytes);
int dm_comm_create(const void* unique_id_128_bytes, int world, int rank, int device_id, dm_comm** out);
int dm_comm_destroy(dm_comm* comm);
/* All-gather `count` floats per rank: recv_dev[r * count ..] = rank r's send_dev.  Enqueued on the comm's own stream, ordered after
 * everything already enqueued on the ctx stream (an event, no host sync), so the caller can launch control step k+1 on the ctx
 * stream right away: the collective overlaps it.  `slot` in [0, 4) names the event pair of this buffer (double buffering). */
int dm_gather_records(dm_ctx* ctx, dm_comm* comm, int slot, const float* send_dev, float* recv_dev, size_t count);
/* Make the ctx stream (not the host) wait for the gather last launched on `slot`; no-op when none is in flight. */
int dm_gather_wait(dm_ctx* ctx, dm_comm* comm, int slot);

/* ---- The reference's random generator, for a host that replays the reference's draw order (the N = 1 drop-in route)
 * cRand (util/Rand.h, util/Rand.cpp:6-135) behind cMathUtil::gRand (util/MathUtil.cpp:6,61-134): std::default_random_engine +
 * the <random> distributions, state kept across calls.  Implemented with the same standard-library types, so a caller that issues
 * the reference's calls in the reference's order -- cDeepMimicCore::SeedRand (DeepMimicCore.cpp:20-23 -> cMathUtil::SeedRand:
 * Seed, then one RandInt for srand), cScene::cScene (scenes/Scene.cpp:5: one RandUint), cTimer::Reset (util/Timer.cpp:55-73),
 * cGround::cGround (sim/Ground.cpp:68: one RandUint), cSceneImitate::CalcRandKinResetTime (scenes/SceneImitate.cpp:494-500) -- gets
 * the reference's reset times and episode limits for the same seed, to hand to dm_reset(kin_times, max_times).  Host only; the
 * batched device path draws from counter-based streams keyed by (seed, global env id, episode) instead. */
typedef struct dm_refrand dm_refrand;
int dm_refrand_create(unsigned long seed, dm_refrand** out);          /* cRand(seed) */
int dm_refrand_destroy(dm_refrand* r);
int dm_refrand_seed(dm_refrand* r, unsigned long seed);               /* cRand::Seed */
double dm_refrand_double(dm_refrand* r, double min, double max);      /* cRand::RandDouble(min, max): min when min == max, no draw */
double dm_refrand_exp(dm_refrand* r, double lambda);                  /* cRand::RandDoubleExp */
double dm_refrand_norm(dm_refrand* r, double mean, double stdev);     /* cRand::RandDoubleNorm */
int dm_refrand_int(dm_refrand* r);                                    /* cRand::RandInt() */
int dm_refrand_int_range(dm_refrand* r, int min, int max);            /* cRand::RandInt(min, max) */
int dm_refrand_uint(dm_refrand* r);                                   /* cRand::RandUint() */
int dm_refrand_discard(dm_refrand* r, long n);                        /* advance the engine by n raw values */
int dm_refrand_norm_state(dm_refrand* r, int set, int* avail, double* saved);    /* the second deviate std::normal_distribution keeps for its next call: read (set = 0) or write */
int dm_refrand_engine_state(dm_refrand* r, int set, unsigned long* state);       /* the engine's state (minstd_rand0: one integer): read or write -- for snapshots */

/* ---- The draw tape: the reference's draw ORDER for the draws that happen on the device (one-env drop-in, `DM_RNG=reference`).
 * The reference draws from two generators -- cMathUtil::gRand ("engine 0": every cTimer::Reset (util/Timer.cpp:55-73), cClipsController::SelectNewMotion
 * (anim/ClipsController.cpp:226-243), cSceneImitate::CalcRandKinResetTime (scenes/SceneImitate.cpp:494-500), the target sampling of strike_amp
 * (scenes/SceneStrikeAMP.cpp:336-383), the ball's rotation angle (scenes/SceneDribbleAMP.cpp:498)) and the scene's own cScene::mRand ("engine 1": goal
 * re-sampling of the task scenes (scenes/SceneHeadingAMP.cpp:168-220, SceneTargetAMP.cpp:275-285, SceneDribbleAMP.cpp:430-520), the random yaw
 * (scenes/SceneImitate.cpp:346), perturbations (scenes/SceneSimChar.cpp:205-256, 952-956), the recovery coin (SceneHeadingAMPGetup.cpp:314)) -- in an order
 * that depends on what happens inside a launch (a target timer running out, a perturbation falling due).  dm_refrand_tape tabulates, for every raw
 * engine position k < DM_TAPE_K past a generator's current state, what each distribution would return if its next call started there (computed with
 * the <random> types themselves); the kernels look their draws up in the reference's call order and advance the two positions; afterwards the host reads
 * the positions back (dm_get_draw_tape_state) and discards that many raw values from its generators (dm_refrand_discard, dm_refrand_norm_state).
 *
 * Row of env e (DM_TAPE_STRIDE doubles): header [0] raw values consumed on engine 0, [1] on engine 1, [2] / [3] engine 1's saved normal deviate
 * (available flag, value), [4] error flag (a launch ran past the tables: raised by the device, the caller must treat the launch as failed),
 * [5] 1 when the kinematic controller is a cClipsController (every reset draws a clip, even out of one), [6..8] the episode timer's
 * {min, max, exp} as cTimer holds them (annealed train-mode parameters whatever the mode; exp <= 0: uniform type), [9] the limit test mode pins
 * after the draws (< 0: none), [10..15] unused; then the tables: engine 0 uniform [K], engine 0 -log(1 - uniform) [K], engine 1 uniform [K],
 * engine 1 normal {value, saved value, raw values consumed} [3 K], engine 1 |RandInt()| {value, raw values consumed} [2 K].
 * With a tape bound, dm_reset without clip times draws the whole reset from it (timers, perturbation clock, clip time, clip, yaw, goal state), and
 * DM_AUTO_RESET is refused.  Contexts without a tape (the batched path) keep their counter-based streams. */
#define DM_TAPE_K 96
#define DM_TAPE_HDR 16
#define DM_TAPE_STRIDE (DM_TAPE_HDR + 8 * DM_TAPE_K)
int dm_refrand_tape(const dm_refrand* r, int K, double* u, double* e, double* n3, double* i2);   /* any table may be null; the generator is not advanced */
int dm_set_draw_tape(dm_ctx* ctx, const double* tape /* N x DM_TAPE_STRIDE; NULL: unbind, back to the counter-based streams */);
int dm_get_draw_tape_state(dm_ctx* ctx, double* out /* N x DM_TAPE_HDR */);
/* the rows of the listed envs only (n x DM_TAPE_STRIDE in, n x DM_TAPE_HDR out): one context serving several one-env callers, each with generators of its own
 * (the shared-owner route, deepmimic_amd/broker.py); every env a launch steps or resets must hold a current row while a tape is bound.  n = 0: bind the
 * rows the device already holds (nothing was drawn from them since they went up). */
int dm_set_draw_tape_envs(dm_ctx* ctx, const int32_t* env_ids, int n, const double* rows);
int dm_get_draw_tape_state_envs(dm_ctx* ctx, const int32_t* env_ids, int n, double* out);

/* ---- Native scene loading: cDeepMimicCore::ParseArgs (DeepMimicCore.cpp:25-44) + the ParseArgs / file loading of the scene classes the path serves,
 * in C++ inside the library (deepmimic_amd/csrc/dm_scene_load.h), so that a native host goes from the reference's own arg file to a running context
 * without Python:   dm_scene_load(args, n, data_root, test_mode, &scene);  dm_create(&info, dm_scene_get_tables(scene), &ctx);
 * `args` are command-line style tokens ("--arg_file", "args/run_humanoid3d_walk_args.txt", or the keys themselves; the first occurrence of a key
 * wins, util/ArgParser.cpp:31-120); relative paths resolve against data_root (the reference resolves them against its working directory).
 * test_mode: the episode timer pinned to time_end_lim_max (scenes/RLSceneSimChar.cpp:277-284).  The tables belong to the scene handle.
 * dm_scene_info out[8] = num_update_substeps, anneal_samples, time_end_lim_min, time_end_lim_max, time_end_lim_exp, time_lim_exp, timer type (0 uniform,
 * 1 exp: call dm_set_timer_exp(ctx, time_lim_exp)), reserved -- what a driver needs beside the tables (SetSampleCount annealing, Update substeps). */
typedef struct dm_scene dm_scene;
int dm_scene_load(const char* const* args, int n_args, const char* data_root, int test_mode, dm_scene** out);
const dm_scene_tables* dm_scene_get_tables(const dm_scene* scene);
int dm_scene_info(const dm_scene* scene, double* out);
int dm_scene_free(dm_scene* scene);

/* ---- On-device policy inference: the actor of learning/pg_agent.py:141-188 with the net of
 * learning/nets/fc_2layers_1024units.py and the normalisers of learning/normalizer.py:95-102, on the matrix cores (bf16
 * operands, fp32 accumulate), so that observation -> action -> control step stays on the GPU.  Weights are fp32 host
 * arrays in tf.layers.dense layout (kernel [in x out] row-major, bias [out]); NULL normaliser / logstd arrays mean
 * identity / 0.  s_clip <= 0: no clipping.  Non-finite observations: with a clip +-inf is clipped like any large value and NaN enters the net
 * as -s_clip; without one the actions of THAT row are unspecified (inf, NaN or finite).  No other row is affected either way. */
typedef struct dm_policy dm_policy;
typedef struct {
    int state_dim, hidden1, hidden2, action_dim;      /* reference: S, 1024, 512, A; hidden widths multiples of 64 */
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float *s_mean, *s_std;                      /* normalize:   (s - mean) / std, clipped to +-s_clip */
    const float *a_mean, *a_std;                      /* unnormalize: norm_a * std + mean */
    const float *logstd;                              /* Gaussian head (learning/tf_distribution_gaussian_diag.py), A entries */
    double s_clip;
} dm_policy_params;
int dm_policy_create(int device_id, const dm_policy_params* params, dm_policy** out);
int dm_policy_destroy(dm_policy* policy);
/* actions[n x A] (and logp[n], optional) for states[n x S]; all DEVICE pointers, asynchronous on hip_stream.
 * sample = 0: the mode (pg_agent.py _mode_a_tf); 1: mean + exp(logstd) * N(0,1) with Philox4x32-10 noise keyed by
 * (seed + env_id_offset + row, step * A + j) -- the generator of deepmimic_amd/streams.py. */
int dm_policy_forward(dm_policy* policy, const float* states_dev, int n, float* actions_dev, float* logp_dev, int sample,
                      uint64_t seed, uint32_t step, int env_id_offset, void* hip_stream);
/* _decide_action of learning/pg_agent.py:214-221 for a batch, with the goal as its own input block:
 *  - goals_dev [n x goal_dim] (RecordGoal): the net's input is the concatenation [state, goal] (pg_agent.py:170-187), so the policy's
 *    state_dim counts the goal columns too (w1 has state_dim rows, s_mean / s_std cover both blocks) and states_dev is n x (state_dim - goal_dim);
 *    goal_dim = 0: as dm_policy_forward;
 *  - exp_rate in [0, 1] (exp_params_curr.rate): with sample = 1 a row takes the sampled action with probability exp_rate (its own coin:
 *    Philox4x32-10 keyed like the noise, counter (step, 1, 0, 0), uniform < exp_rate) and the mode otherwise; logp is the one of the action
 *    taken; exp_flags_dev[n] (optional, int32) = 1 for the rows that explored (the EXP flag of a path's steps, pg_agent.py:251-255). */
int dm_policy_forward_ex(dm_policy* policy, const float* states_dev, const float* goals_dev, int goal_dim, int n, float* actions_dev,
                         float* logp_dev, int32_t* exp_flags_dev, double exp_rate, int sample, uint64_t seed, uint32_t step, int env_id_offset,
                         void* hip_stream);
/* Which kernels a forward call ran (deepmimic_amd/csrc/dm_policy_host.h policy_path, the one function every launch goes through):
 * the one-launch actor k_policy_fused<K1 / 32, N3 / 16> where it is compiled for the widths (1024, 512, K1 256 / 384, N3 32 / 64), else k_policy_prep +
 * one kernel per layer: layers 1 and 2 each on the one-wave kernel (k_policy_layer<0,4,4> / <1,2,4>) or on the LDS-tiled GEMM with 64- or 128-row
 * tiles (k_policy_gemm<layer, 64 | 128>), then k_policy_layer<2,1,2>.  A per-layer id is DM_POLICY_PATH_LAYERED(layer-1 choice, layer-2 choice). */
enum { DM_POLICY_LAYER_ONE_WAVE = 0, DM_POLICY_LAYER_TILE64 = 1, DM_POLICY_LAYER_TILE128 = 2 };
#define DM_POLICY_PATH_LAYERED_BASE 16
#define DM_POLICY_PATH_LAYERED(l1, l2) (DM_POLICY_PATH_LAYERED_BASE + (l1) + 4 * (l2))
#define DM_POLICY_PATH_LAYER1(path) (((path) - DM_POLICY_PATH_LAYERED_BASE) & 3)
#define DM_POLICY_PATH_LAYER2(path) (((path) - DM_POLICY_PATH_LAYERED_BASE) >> 2)
enum dm_policy_path {
    DM_POLICY_PATH_NONE = -1,                /* no forward call yet */
    DM_POLICY_PATH_FUSED_8_2 = 0,            /* k_policy_fused<8, 2>:  K1 = 256, N3 = 32 */
    DM_POLICY_PATH_FUSED_8_4 = 1,            /* k_policy_fused<8, 4>:  K1 = 256, N3 = 64 */
    DM_POLICY_PATH_FUSED_12_2 = 2,           /* k_policy_fused<12, 2>: K1 = 384, N3 = 32 */
    DM_POLICY_PATH_FUSED_12_4 = 3,           /* k_policy_fused<12, 4>: K1 = 384, N3 = 64 */
    DM_POLICY_PATH_WAVE_WAVE = 16,           /* layer<0,4,4>, layer<1,2,4>: DM_POLICY_ONE_WAVE, or neither hidden width a multiple of 128 */
    DM_POLICY_PATH_TILE64_WAVE = 17,         /* gemm<0,64>,   layer<1,2,4> */
    DM_POLICY_PATH_TILE128_WAVE = 18,        /* gemm<0,128>,  layer<1,2,4> */
    DM_POLICY_PATH_WAVE_TILE64 = 20,         /* layer<0,4,4>, gemm<1,64> */
    DM_POLICY_PATH_TILE64_TILE64 = 21,       /* gemm<0,64>,   gemm<1,64>: the per-layer default at 1024 / 512 */
    DM_POLICY_PATH_WAVE_TILE128 = 24,        /* layer<0,4,4>, gemm<1,128> */
    DM_POLICY_PATH_TILE128_TILE128 = 26      /* gemm<0,128>,  gemm<1,128>: DM_POLICY_TILE=128 */
};
/* out[0] = K1 and out[1] = N3, the padded input / action widths the context really uses; out[2] = 1 if it holds a fused weight stream;
 * out[3] = dm_policy_path of the LAST dm_policy_forward(_ex) on this context (DM_POLICY_PATH_NONE before any; the environment switches
 * DM_POLICY_LAYERED / DM_POLICY_ONE_WAVE / DM_POLICY_TILE are read per call); out[4] = its row count; out[5] = 1 for a gated context
 * (dm_policy_create_gated), out[6] = its goal_dim, out[7] = 1 if the fused stream it holds is the gated one */
int dm_policy_info(dm_policy* policy, int32_t* out);

/* The gated actor of the AMP task policies (learning/nets/fc_2layers_gated_1024units.py, "ActorNet": "fc_2layers_gated_1024units"): a small net on the
 * NORMALISED GOAL, the last goal_dim input columns, scales and shifts the pre-activations of both hidden layers --
 *   c = relu(Wc xg + bc);  e_i = relu(We_i c + be_i);  beta_i = Wb_i e_i + bb_i;  sigma_i = 2 sigmoid(Ws_i e_i + bs_i);  h_i = relu(sigma_i * (W_i h + b_i) + beta_i)
 * -- head, noise, exploration coin and logp as in the plain actor.  Arrays in tf.layers.dense layout like dm_policy_params: gc_* = actor/gate_common/0/dense
 * [goal_dim x gate_common]; g{i}_w / _b = actor/gate{i}/0/dense [gate_common x gate_hidden]; g{i}_bias_* = actor/gate{i}/dense and g{i}_scale_* =
 * actor/gate{i}/dense_1, [gate_hidden x hidden1] for i = 0 and [gate_hidden x hidden2] for i = 1.  Refused at create: goal_dim outside [1, min(state_dim - 1, 128)],
 * gate widths that are no multiples of 32, gate_common > 256, gate_hidden > 128 (reference: 128, 64).
 * The result is an ordinary dm_policy: dm_policy_forward(_ex), dm_policy_bind_obs_normalizer (g_norm bound at column state_dim - goal_dim feeds the gate with no
 * further call), dm_policy_info and dm_policy_destroy work on it.  dm_policy_forward_ex takes goal_dim equal to the gate's with a goal block, or goal_dim = 0
 * with the goal in the last columns of states_dev; any other goal_dim fails.  Which kernels run is (dm_policy_path id, gated): the id says which kernel serves
 * each layer, out[5] of dm_policy_info that its GATED instantiation ran: k_policy_fused<.., true> in one launch at 1024 / 512, K1 256 / 384, N3 32 / 64 with
 * gate_hidden = 64 (out[2] = out[7] = 1), else -- and under DM_POLICY_LAYERED -- k_policy_gate and the GATED per-layer kernels.  Rounding points:
 * deepmimic_amd/csrc/dm_policy.h GateDev. */
typedef struct {
    int goal_dim, gate_common, gate_hidden;
    const float *gc_w, *gc_b;
    const float *g0_w, *g0_b, *g0_bias_w, *g0_bias_b, *g0_scale_w, *g0_scale_b;
    const float *g1_w, *g1_b, *g1_bias_w, *g1_bias_b, *g1_scale_w, *g1_scale_b;
} dm_policy_gate_params;
int dm_policy_create_gated(int device_id, const dm_policy_params* params, const dm_policy_gate_params* gate, dm_policy** out);

/* New weights into a live context, in place: ONE kernel launch on hip_stream (k_policy_pack, deepmimic_amd/csrc/dm_policy.h) rounds the fp32 arrays to bf16
 * (round to nearest even, NaN -> 0x7fc0) and scatters them into the fragment layouts the forward kernels read -- w1p / w2p / w3p, the fused stream, the gate's
 * arrays and the gated fused stream with its interleaved scale / bias vectors -- in the buffers dm_policy_create(_gated) allocated, byte for byte what create
 * makes of the same arrays.  A learner whose parameters live on the device calls it after every optimiser step instead of destroy + create.
 *  - params / gate: the structs of create.  The widths (state_dim, hidden1, hidden2, action_dim; goal_dim, gate_common, gate_hidden) must equal the context's,
 *    else an error names the mismatch and nothing is written.  gate must be non-NULL exactly when the context is gated.
 *  - a NULL array keeps what the context holds (only logstd, only the three layers, ...).  s_mean / s_std become s_mean / 1 / s_std; s_clip is ignored and
 *    stays as created; K1 / N3 and the choice of kernels stay what create made them (dm_policy_info).
 *  - flags: DM_DEVICE_PTRS -- the arrays are DEVICE pointers (4-byte alignment is enough: views of a torch tensor); the call then allocates nothing, copies
 *    nothing from the host and does not synchronise: it may be enqueued between two dm_policy_forward on one stream, and the second one sees the new weights.
 *    Without it they are host arrays, staged through one device temporary of the call; the call then synchronises hip_stream.
 *    DM_WEIGHTS_OUT_IN -- every 2-D array is [out x in] row-major (torch.nn.Linear.weight) instead of [in x out] (tf.layers.dense); vectors are the same.
 *  - ordering is the caller's: the refresh is ordered on hip_stream like every other call here.  A forward on ANOTHER stream that overlaps it reads a mixture
 *    of old and new weights; so does a bound normaliser copy (dm_policy_bind_obs_normalizer) racing a refresh of s_mean / s_std. */
enum { DM_WEIGHTS_OUT_IN = 32 };            /* shares the flag word of DM_DEVICE_PTRS */
int dm_policy_set_weights(dm_policy* policy, const dm_policy_params* params, const dm_policy_gate_params* gate, int flags, void* hip_stream);
/* One packed DEVICE array of the context to the host, as the kernels read it (tests, diagnosis): *bytes = its size; host_out = NULL asks for the size only,
 * else capacity must cover it.  Synchronises the device first.  DM_POLICY_PACKED_WFS fails on a context without a fused stream (out[2] of dm_policy_info),
 * the gate ids on a context without a gate.  Sizes: w1p K1 x hidden1, w2p hidden1 x hidden2, w3p hidden2 x N3 bf16 in [n-tile][k-step][lane][8] order;
 * b3 N3 floats (zero-padded); s_inv_std = 1 / s_std; gate ids per gated layer i in the order of dm_policy_gate_params. */
enum dm_policy_packed {
    DM_POLICY_PACKED_W1P = 0, DM_POLICY_PACKED_W2P, DM_POLICY_PACKED_W3P, DM_POLICY_PACKED_B1, DM_POLICY_PACKED_B2, DM_POLICY_PACKED_B3,
    DM_POLICY_PACKED_S_MEAN, DM_POLICY_PACKED_S_INV_STD, DM_POLICY_PACKED_A_MEAN, DM_POLICY_PACKED_A_STD, DM_POLICY_PACKED_LOGSTD, DM_POLICY_PACKED_WFS,
    DM_POLICY_PACKED_GATE_WCP = 16, DM_POLICY_PACKED_GATE_BC,                                       /* gc_w (KG x gate_common, KG = goal_dim rounded up to 32), gc_b */
    DM_POLICY_PACKED_GATE_WEP0, DM_POLICY_PACKED_GATE_BE0, DM_POLICY_PACKED_GATE_WBP0, DM_POLICY_PACKED_GATE_BB0, DM_POLICY_PACKED_GATE_WSP0, DM_POLICY_PACKED_GATE_BS0,
    DM_POLICY_PACKED_GATE_WEP1, DM_POLICY_PACKED_GATE_BE1, DM_POLICY_PACKED_GATE_WBP1, DM_POLICY_PACKED_GATE_BB1, DM_POLICY_PACKED_GATE_WSP1, DM_POLICY_PACKED_GATE_BS1
};
int dm_policy_read_packed(dm_policy* policy, int which, void* host_out, size_t capacity, size_t* bytes);

/* ---- Scalar heads of the device nets: the critic (learning/pg_agent.py:161-171: the actor's two-layer net with a one-unit linear output on [norm_s, norm_g];
 * gated in the AMP task agents) and the AMP discriminator (learning/amp_agent.py:178-194: fc_2layers_1024units on amp_obs_norm-normalised observations, output
 * disc_logits).  A scalar context IS a policy context with action_dim = 1: dm_policy_create / dm_policy_create_gated (a_mean, a_std, logstd may be NULL),
 * dm_policy_set_weights, dm_policy_bind_obs_normalizer, dm_policy_read_packed and dm_policy_destroy work on it.  dm_policy_eval_scalar takes n observation rows
 * (states_dev / goals_dev / goal_dim as dm_policy_forward_ex) to the finished per-row scalar in out_dev[n] in ONE launch where the one-launch kernel is compiled
 * for the widths (else the per-layer kernels with the head in the last): no noise is drawn, logstd / a_mean / a_std are not read, nothing like logp is written.
 * With y = the net's output (bf16 operands, fp32 accumulation: bit for bit the mode action of an actor built from the same arrays):
 *   DM_SCALAR_HEAD_VALUE   v = min(max(y, lo), hi) -- the AMP agent's value clip (amp_agent.py:441-443), infinite bounds give PPO's behaviour; a NaN y gives lo --
 *                          then, with terminate_dev (int32 per row, eTerminate), v = val_fail where it is 1 (Fail) and val_succ where it is 2 (Succ)
 *                          (ppo_agent.py:262-264);
 *   DM_SCALAR_HEAD_STYLE   d = 1 - y, r = scale * max(0, 1 - 0.25 d^2) (amp_agent.py:393-434), then, with task_reward_dev (float per row),
 *                          r = (1 - lerp) r + lerp task_r (amp_agent.py:294-297), lerp in [0, 1]; fp32, every multiply-add one fma.
 * row_mask_dev (int32 per row, optional): a row whose flag is 0 gets `fill` in out_dev and raw_out_dev.  In the one-launch kernel a whole 32-row tile of such
 * rows leaves before its first weight request, so it costs a launch slot and 32 flag reads -- critic values on terminal observations are read only where the
 * step was done.  LIMIT: on the per-layer route (widths without a one-launch kernel, or DM_POLICY_LAYERED=1) only the last launch, the layer-3 head kernel,
 * honours the mask (16-row tiles); k_policy_prep, k_policy_gate and layers 1 and 2 still run for every row, so masking saves next to nothing there.
 * raw_out_dev (optional, n floats): y itself, for the discriminator's logit statistics.  Rows [0, n) of the outputs are always written, nothing else is.
 * Asynchronous on hip_stream; no allocation beyond the activation buffers a context grows to its largest n.  Fails on a context whose action_dim is not 1. */
enum { DM_SCALAR_HEAD_VALUE = 0, DM_SCALAR_HEAD_STYLE = 1 };
typedef struct {
    int kind;                           /* DM_SCALAR_HEAD_VALUE / DM_SCALAR_HEAD_STYLE */
    float lo, hi;                       /* value: clip bounds (-inf / +inf: none) */
    float val_fail, val_succ;           /* value: what a Fail / Succ row gets with terminate_dev */
    const int32_t* terminate_dev;       /* value: n flags or NULL */
    float scale, lerp;                  /* style: reward_scale, task_reward_lerp */
    const float* task_reward_dev;       /* style: n task rewards or NULL (then lerp is not used) */
    const int32_t* row_mask_dev;        /* n flags or NULL (every row) */
    float fill;                         /* what a masked-out row gets */
} dm_scalar_head;
int dm_policy_eval_scalar(dm_policy* policy, const float* states_dev, const float* goals_dev, int goal_dim, int n, const dm_scalar_head* head,
                          float* out_dev, float* raw_out_dev, void* hip_stream);
/* the LAST dm_policy_eval_scalar on this context: out[0] = the dm_policy_path id that served it (the HEAD instantiation of the kernel that holds layer 3;
 * DM_POLICY_PATH_NONE before any), out[1] = its row count, out[2] = its head kind, out[3] = 1 if it had a row mask.  dm_policy_info keeps reporting the last
 * dm_policy_forward(_ex) only. */
int dm_policy_scalar_info(dm_policy* policy, int32_t* out);

/* ---- Running observation statistics on the device: the Normalizer of the reference's learner (learning/normalizer.py:6-152; the
 * s_norm / g_norm / amp_obs_norm of learning/rl_agent.py:466-483, amp_agent.py:290-291) for records that stay in HBM.
 * group_ids (NULL = one NORM_GROUP_SINGLE group): per column -1 = never updated (NORM_GROUP_NONE), 0 = per element, k > 0 = the
 * columns of group k share the average of the new data (normalizer.py:141-149; dm_build_offsets_scales hands the ids out).
 * eps = smallest std (reference: 0.02); clip <= 0 or inf = no clipping in dm_norm_normalize. */
typedef struct dm_normalizer dm_normalizer;
int dm_norm_create(int device_id, int size, const int32_t* group_ids, double eps, double clip, dm_normalizer** out);
int dm_norm_destroy(dm_normalizer* norm);
/* Normalizer.record (normalizer.py:33-45): new_count += n, new_sum += column sums, new_sum_sq += column sums of squares, in fp64, of
 * x[n x size] fp32 -- a DEVICE pointer with DM_DEVICE_PTRS in flags (the record block of a control step), a host pointer otherwise.
 * Asynchronous on hip_stream; deterministic (two passes, no atomics). */
int dm_norm_record(dm_normalizer* norm, const float* x, int n, int flags, void* hip_stream);
/* the pending sums {new_count, new_sum[size], new_sum_sq[size]} as ONE device array of 1 + 2 size doubles: what MPIUtil.reduce_sum
 * (normalizer.py:48-50) adds over the workers -- all-reduce it (SUM) over the ranks before dm_norm_update */
int dm_norm_pending(dm_normalizer* norm, double** dev_ptr, int* len);
/* Normalizer.update (normalizer.py:47-73): fold the pending sums into count / mean / mean_sq / std, clear them.  Asynchronous on hip_stream. */
int dm_norm_update(dm_normalizer* norm, void* hip_stream);
/* set_mean_std (normalizer.py:79-93; host arrays): mean_sq = std^2 + mean^2; count >= 0 also sets the sample count (TFNormalizer.load), < 0 keeps it */
int dm_norm_set(dm_normalizer* norm, const double* mean, const double* std, int64_t count, void* hip_stream);
/* host copies of the statistics (any pointer may be NULL); synchronises hip_stream */
int dm_norm_get(dm_normalizer* norm, double* mean, double* std, double* mean_sq, int64_t* count, void* hip_stream);
/* what dm_norm_get handed out, put back word for word (host arrays; a learner's checkpoint): mean_sq is stored as given, not rebuilt from std as dm_norm_set
 * does, so the next dm_norm_update continues from the saved bits.  count >= 0, std > 0. */
int dm_norm_set_state(dm_normalizer* norm, const double* mean, const double* std, const double* mean_sq, int64_t count, void* hip_stream);
/* Normalizer.normalize (normalizer.py:95-98) of x[n x size] into out[n x size], DEVICE pointers, fp32 */
int dm_norm_normalize(dm_normalizer* norm, const float* x_dev, int n, float* out_dev, void* hip_stream);
/* make `norm` columns [first_column, first_column + size) of the observation normaliser of `policy` (a device-to-device copy of mean and 1 / std,
 * ordered on hip_stream): the actor's next dm_policy_forward on that stream normalises with the statistics of the last dm_norm_update / dm_norm_set.
 * s_norm at column 0 and g_norm at column state_size, as the reference keeps them (learning/rl_agent.py:212-222). */
int dm_policy_bind_obs_normalizer(dm_policy* policy, dm_normalizer* norm, int first_column, void* hip_stream);

/* ---- TD(lambda) returns over a device-resident rollout: RLUtil.compute_return (learning/rl_util.py:3-18) per path with the end-of-path rules of
 * learning/ppo_agent.py:251-284, for T control steps of N envs that stayed in HBM.  All arrays are DEVICE pointers, time-major (row t = the N envs'
 * values of step t, the way a sampler stacks TorchVecEnv's outputs): rewards T x N; values (T + 1) x N, values[t] = the critic on the observation the
 * action of step t was taken from, values[T] = the critic on the observation after the last step; term_values T x N, the critic on the terminal
 * observation of step t (dm_set_terminal_outputs), used only where done[t] != 0; terminate (eTerminate), done (the env was reset in step t:
 * episode_end != 0 or valid == 0) and valid (NULL = every episode valid), T x N int32 each.  Per env column, backwards in time, the value behind step t is
 * v_next = values[t + 1] if the step is not done, val_fail / val_succ if it is done with terminate Fail / Succ, term_values[t] if it is done with Null;
 * a step that closes a path (done, or t = T - 1) gets ret = r + gamma v_next, any other ret = r + gamma ((1 - td_lambda) v_next + td_lambda ret[t + 1]):
 * fp64 arithmetic on the fp32 inputs in the reference's association, rounded once into returns (T x N floats).  gamma = 0 gives the rewards back
 * (ppo_agent.py:269-270).  mask (T x N int32, NULL = not wanted): 0 for every step of an episode that ended with valid == 0 inside the window, back to
 * the previous done or to t = 0 -- the reference's driver discards such an episode --, 1 elsewhere.
 * ONE DEVIATION: the reference stores whole paths only; a rollout window cut at T is bootstrapped from values[T] like a Null path end, and a path that
 * began before the window starts at row 0.  Advantages, value clipping and their normalisation stay the caller's (one-line tensor ops).
 * Needs no dm_ctx; asynchronous on hip_stream of device device_id.  T < 1, N < 1 or a NULL required pointer: error, nothing is launched. */
int dm_td_lambda_returns(int device_id, int T, int N, const float* rewards_dev, const float* values_dev, const float* term_values_dev,
                         const int32_t* terminate_dev, const int32_t* done_dev, const int32_t* valid_dev, double gamma, double td_lambda,
                         double val_fail, double val_succ, float* returns_dev, int32_t* mask_dev, void* hip_stream);

/* ---- PPO training batches from a device-resident rollout: what PPOAgent._train_step (learning/ppo_agent.py:141-232) does between the returns and the first
 * optimiser step.  Stateless like dm_td_lambda_returns: DEVICE pointers, time-major T x N arrays addressed by the flat index i = t * N + n, asynchronous on
 * hip_stream of device device_id, no allocation and no synchronisation inside; a refused call launches nothing.
 *
 * dm_ppo_advantages.  returns T x N and mask T x N (NULL: all 1) as dm_td_lambda_returns wrote them; values: the first T rows of its (T + 1) x N values
 * array; exp_flags T x N as dm_policy_forward_ex wrote them (NULL: every step explored).  Sample i is VALID where mask[i] != 0 and EXP where it is valid and
 * exp_flags[i] != 0.  All arithmetic is fp64 on the fp32 inputs with one rounding to fp32 at a store:
 *   counts_out int32[2] = {n_valid, n_exp};  valid_idx_out / exp_idx_out int32[T * N]: the flat indices of the valid / exp samples in ascending order
 *   (entries from the count on are left untouched);
 *   stats_out double[2] = {mean, std} of a_i = returns[i] - values[i] over the exp samples: std is the population standard deviation taken in two passes
 *   (the mean, then the squared deviations; never E[x^2] - E[x]^2); both are 0 when n_exp == 0;
 *   adv_out T x N = clip((a_i - mean) / (std + adv_eps), -norm_adv_clip, +norm_adv_clip) on exp samples, exactly 0 elsewhere (ppo_agent.py:166-172:
 *   ADV_EPS = 1e-5, NormAdvClip 5);  targets_out T x N = clip(returns[i], val_min, val_max) for every i (:167; infinite bounds: no clip).
 * Sums and the compaction go through per-workgroup partials in `workspace` (dm_ppo_workspace_bytes(T, N) bytes, the caller's, 8-byte aligned like
 * stats_out) folded in a fixed order by further launches: no atomics, no workgroup waits on another one, and two calls on one input are bit-identical.
 * Refused: T < 1, N < 1, T * N > 2^31 - 1, a NULL pointer other than mask / exp_flags, a workspace that is too small, adv_eps < 0, norm_adv_clip <= 0,
 * val_min > val_max. */
int64_t dm_ppo_workspace_bytes(int T, int N);          /* < 0: refused (dm_last_error) */
int dm_ppo_advantages(int device_id, int T, int N, const float* returns_dev, const float* values_dev, const int32_t* mask_dev, const int32_t* exp_flags_dev,
                      double adv_eps, double norm_adv_clip, double val_min, double val_max, float* adv_out, float* targets_out, int32_t* valid_idx_out,
                      int32_t* exp_idx_out, int32_t* counts_out, double* stats_out, void* workspace, int64_t workspace_bytes, void* hip_stream);
/* dm_ppo_gather: rows of a shuffled pass over one of the two lists, one launch for up to 8 columns.  idx_dev: valid_idx_out or exp_idx_out; count_dev: the
 * list's DEVICE-resident counter (&counts_out[0] or &counts_out[1]) -- the host never reads it.  A column is a (T * N) x width array of 4-byte elements
 * (float or int32; width = the product of the trailing dimensions, >= 1) and dst is rows x width.  For j in [0, rows): position p = first + j, pass = p / count,
 * slot = p % count, source row = idx[perm(count, seed, epoch, pass)(slot)] -- a list shorter than the positions asked of it wraps like np.mod(batch, num_idx)
 * (ppo_agent.py:186-193), and every wrap and every epoch sees a fresh shuffle (:190, 211).  picked_out int32[rows] (NULL: not wanted) receives the source rows.
 * count == 0: dst is left untouched and picked_out gets -1.
 * perm is a keyed bijection on [0, count), evaluated per row (nothing is stored or sorted): k = max(1, bit_length(count - 1)), h = ceil(k / 2), m = 2^h - 1;
 * x = (L, R) = (x >> h, x & m); six rounds (L, R) <- (R, L xor (F & m)), F = word 0 of Philox4x32-10(counter = (R, round, epoch, pass mod 2^32),
 * key = (seed & 0xffffffff, seed >> 32)); y = (L << h) | R, and while y >= count the six rounds are applied to y again (deepmimic_amd/ppo_batch.py
 * reference_permutation is the same in numpy).
 * Rows are copied as dwords, coalesced; 16 bytes per lane only where src, dst and width * 4 are all multiples of 16.  The source rows are not bounds-checked:
 * idx must hold row numbers of the columns passed.  Refused: a NULL idx / count / column pointer, first < 0, rows < 1, ncols outside 1 .. 8, width < 1. */
typedef struct dm_ppo_column { const void* src; void* dst; int32_t width; } dm_ppo_column;
int dm_ppo_gather(int device_id, const int32_t* idx_dev, const int32_t* count_dev, int64_t first, int rows, uint64_t seed, uint32_t epoch, int ncols,
                  const dm_ppo_column* cols, int32_t* picked_out, void* hip_stream);

/* ---- replay stores for the AMP discriminator's data (deepmimic_amd/csrc/dm_replay.h, deepmimic_amd/replay.py): the reference's ReplayBufferRandStorage
 * (learning/replay_buffer_rand_storage.py; learning/amp_agent.py:70-77, 216-227) on arrays that never leave HBM.  Stateless on the library side: the caller owns
 * buf [capacity, width] of 4-byte elements (float or int32) and state, an int64[2] = {size, total} on the device; {0, 0} is a cleared store.  Asynchronous on
 * hip_stream (NULL: the null stream) of device_id, no host read, no atomics; the same (state, seed, call, inputs) give the same bytes.
 *
 * dm_replay_append: n = min(*count_dev, max_rows), read on the device (count_dev NULL: n = max_rows; e.g. &counts_out[0] of dm_ppo_advantages with idx_dev =
 * valid_idx_out).  With old = size and free = capacity - old, list row j < n has the rank q = j when n <= capacity and q = perm(n, seed, call, 0x494E43)(j)
 * otherwise (a rollout larger than the store keeps a uniformly chosen subset), and goes to the slot
 *     old + q                                     q < free                  (free slots first)
 *     perm(old, seed, call, 0x564943)(q - free)   free <= q < capacity      (distinct old rows, as np.random.choice(curr_size, remainder, replace=False))
 *     nowhere                                     q >= capacity             (dropped)
 * perm(count, seed, epoch, pass) is the keyed bijection of dm_ppo_gather above.  Source row idx_dev[j] of src_dev (idx_dev NULL: row j) is copied to its slot, and,
 * when packed_out [max_rows, width] is given, to packed_out[j] for every j < n, dropped rows included (the dense rows a normaliser records).  slots_out int32[max_rows]
 * (NULL: not wanted) receives the slot, -1 for a dropped row.  Rows j >= n of both outputs are not touched.  All slots of one call are distinct.  The new state,
 * size = min(old + n, capacity) and total += n, is written by a one-thread launch behind the copy.  Rows are copied as dwords, coalesced; 16 bytes per lane only
 * where buf, src, packed_out and width * 4 are all multiples of 16.  The source rows are not bounds-checked.
 *
 * dm_replay_sample: with size = state[0], destination row r of dst_dev [rows, width] reads slot mulhi32(w, size), w = word 0 of Philox4x32-10(counter =
 * (r, call, 0x534D50, 0), key = (seed & 0xffffffff, seed >> 32)): with replacement, as np.random.randint(0, curr_size, n).  picked_out int32[rows] (NULL: not
 * wanted) receives the slots.  size == 0: dst is left untouched and picked_out gets -1.
 *
 * Refused: a NULL buf / state / src / dst; capacity, width, max_rows or rows < 1; capacity * width, max_rows * width or rows * width above 2^31 - 1; a pointer that
 * is not 4-byte aligned; state not 8-byte aligned; no HIP device, or a device_id it does not have. */
int dm_replay_append(int device_id, void* buf_dev, int capacity, int width, int64_t* state_dev, const void* src_dev, const int32_t* idx_dev /* NULL: row j = j */,
                     const int32_t* count_dev /* NULL: n = max_rows */, int max_rows, uint64_t seed, uint32_t call, void* packed_out /* NULL, or [max_rows, width] */,
                     int32_t* slots_out /* NULL, or [max_rows] */, void* hip_stream);
int dm_replay_sample(int device_id, const void* buf_dev, int width, const int64_t* state_dev, int rows, uint64_t seed, uint32_t call, void* dst_dev /* [rows, width] */,
                     int32_t* picked_out /* NULL or [rows] */, void* hip_stream);

/* ---- episode returns, lengths and end-cause totals over a device-resident rollout (deepmimic_amd/csrc/dm_episode.h, deepmimic_amd/episodes.py): what the reference's
 * learner logs as Train_Return / Test_Return -- path.calc_return() of the finished, valid paths (learning/path.py:45-46, learning/rl_agent.py:351-365, 456-466); a path
 * with a non-finite value is never stored (learning/replay_buffer.py:102-112), an invalid episode is discarded by the driver.  Stateless like dm_td_lambda_returns:
 * DEVICE pointers, time-major T x N arrays (rewards float; terminate, done, valid int32, valid NULL = every episode valid), the caller owns every byte of state,
 * asynchronous on hip_stream of device device_id, no allocation, no host read and no synchronisation inside; a refused call launches nothing.  T = 1 is the per-step
 * use, T = the rollout length the per-iteration use.
 *
 * Per env column n, forward in time, on the carry acc_return[n] (double) / acc_len[n] (int32), both in/out ({0, 0}: no episode in flight):
 *   step t:  acc_return += (double)rewards[t] (fp64, in time order, no contraction), acc_len += 1;  then ep_return_out[t] = (float)acc_return and
 *            ep_len_out[t] = acc_len (each NULL = not wanted): the running return and length of the episode step t belongs to, step t included -- at a done step the
 *            finished episode's figures; one rounding to fp32, at the store.
 *   where done[t] != 0 the episode finishes with class c = 3 (invalid) if valid[t] == 0 or acc_return is not finite (an fp64 sum of fp32 rewards is non-finite exactly
 *            when a reward was: path.check_vals), else c = terminate[t] if that is 1 (Fail) or 2 (Succ), else c = 0 (Null: episode timer, clip end -- the rule of
 *            dm_td_lambda_returns); then both accumulators of the column go to zero.
 * After the call the carry holds the accumulators behind step T - 1: an episode that began before the window is counted with what the carry held, one still running
 * at T stays in the carry and is not counted.
 *
 * totals_dev (NULL = not wanted): DM_EP_TOTALS_WORDS 8-byte words, ADDED TO by every call; a window starts from the initial block, all zero bits except
 * ret_min = +inf and ret_max = -inf.  int64 words: DM_EP_EPISODES + c, DM_EP_STEPS + c (sum of the lengths), DM_EP_LEN_MAX + c for c in 0 .. 3, and
 * DM_EP_STEPS_SEEN (+= T * N per call).  fp64 words, c in 0 .. 2 only (class 3 keeps counts: its returns may be NaN and are what the reference throws away):
 * DM_EP_RET_SUM + c, DM_EP_RET_SQ + c (sum of squares), DM_EP_RET_MIN + c, DM_EP_RET_MAX + c, all of the fp64 acc_return, not of the rounded float.
 * hist_dev (NULL = not wanted; then bins and bin_steps are ignored): int64[bins], added to: a finished episode of class < 3 and length L adds 1 to bin
 * min((L - 1) / bin_steps, bins - 1).
 * Each workgroup folds its columns' totals by a fixed tree and writes one partial block to work_dev (dm_episode_workspace_bytes(N) bytes, the caller's); a second
 * one-workgroup launch behind it folds the partials in workgroup order into totals_dev.  Histogram counts are integer atomic adds.  No floating-point atomic, no
 * workgroup waits on another one: integer results are exact, every fp64 sum has one order for given (T, N), two calls on the same inputs give the same bytes.  With
 * totals_dev NULL the second launch is skipped; with totals_dev and hist_dev both NULL work_dev may be NULL.
 * Refused: T < 1, N < 1, T * N > 2^31 - 1; a NULL rewards / terminate / done / acc_return / acc_len; hist_dev with bins < 1 or bin_steps < 1; totals or a histogram
 * with work_bytes < dm_episode_workspace_bytes(N); acc_return, totals, hist or (where used) the workspace not 8-byte aligned; no HIP device or a device_id it does not have. */
enum { DM_EP_EPISODES = 0, DM_EP_STEPS = 4, DM_EP_LEN_MAX = 8, DM_EP_RET_SUM = 12, DM_EP_RET_SQ = 15, DM_EP_RET_MIN = 18, DM_EP_RET_MAX = 21, DM_EP_STEPS_SEEN = 24,
       DM_EP_TOTALS_WORDS = 25 };
enum { DM_EP_NULL = 0, DM_EP_FAIL = 1, DM_EP_SUCC = 2, DM_EP_INVALID = 3 };      /* the episode classes c */
int64_t dm_episode_workspace_bytes(int N);             /* < 0: refused (dm_last_error) */
int dm_episode_stats(int device_id, int T, int N, const float* rewards_dev, const int32_t* terminate_dev, const int32_t* done_dev,
                     const int32_t* valid_dev /* NULL: all valid */, double* acc_return_dev /* [N] in/out */, int32_t* acc_len_dev /* [N] in/out */,
                     float* ep_return_out /* NULL or [T, N] */, int32_t* ep_len_out /* NULL or [T, N] */, void* totals_dev /* NULL or DM_EP_TOTALS_WORDS words, in/out */,
                     int64_t* hist_dev /* NULL or [bins], in/out */, int bins, int bin_steps, void* work_dev, int64_t work_bytes, void* hip_stream);

/* ---- AMP batch rewards, reward statistics and the critic's value bounds over a device-resident rollout (deepmimic_amd/csrc/dm_amp_rewards.h,
 * deepmimic_amd/amp_rewards.py): AMPAgent._batch_calc_reward (learning/amp_agent.py:393-421), _lerp_reward (:423-425) and the value clip of _compute_batch_vals
 * (:436-443).  At train time the reference scores the WHOLE stored rollout with the discriminator as it is after _update_disc and clips the critic's values to the
 * RUNNING extrema of that reward over 1 - discount.  Stateless like dm_td_lambda_returns: DEVICE pointers, time-major T x N arrays addressed by the flat index
 * i = t * N + n, asynchronous on hip_stream of device device_id, no allocation, no host read, no synchronisation and no atomics inside; a refused call launches
 * nothing, writes nothing and names its reason through dm_last_error.
 *
 * dm_amp_batch_rewards.  logits T x N: the discriminator's y (raw_out_dev of dm_policy_eval_scalar); task_reward T x N or NULL; done, valid T x N int32 (valid NULL:
 * every episode valid, and done is then not read and may be NULL too).  reward_scale and task_reward_lerp are rounded to the floats a dm_scalar_head holds.
 *   rewards_out T x N, EVERY row, counted or not: bit for bit what the DM_SCALAR_HEAD_STYLE head writes from the same logit (one device function serves both):
 *     d = 1 - y;  s = fmaxf(fmaf(-0.25f * d, d, 1.0f), 0.0f) * scale;  r = fmaf(lerp, task_r, (1.0f - lerp) * s) with a task reward, r = s without.
 *   mask_out T x N int32 (NULL: not wanted): exactly the mask of dm_td_lambda_returns from the same done / valid -- 0 for the steps of an episode that ended with
 *     valid == 0 inside the window, back to the previous done or to t = 0, 1 elsewhere (an episode still running at T included).  It depends on the flags alone.
 *     A row is COUNTED where the mask is 1.
 *   stats_out double[DM_AMP_STATS_WORDS], over the counted rows: DM_AMP_STAT_N their number; DM_AMP_STAT_MEAN / DM_AMP_STAT_STD the mean and the POPULATION standard
 *     deviation of s, the scaled style term before the blend (Disc_Reward_Mean / Disc_Reward_Std, amp_agent.py:400-403), in two passes (the mean, then the squared
 *     deviations), fp64 from the fp32 values, no product contracted into a sum; DM_AMP_STAT_MIN / DM_AMP_STAT_MAX this call's min and max of r.  n = 0: mean = std = 0,
 *     min = +inf, max = -inf.
 *   bounds float[2], in/out: bounds[0] = min(bounds[0], cur_min), bounds[1] = max(bounds[1], cur_max); the initial state is {+inf, -inf} (amp_agent.py:46-47);
 *     n = 0 leaves them untouched.  Every min / max here keeps a NaN, as np.amin / np.minimum do: a NaN r in a counted row makes this call's min and max, and with them
 *     both bounds, NaN (and stays: a non-finite input remains visible); rows that are not counted reach neither the bounds nor the statistics.
 * Order of every fp64 sum, fixed for given (T, N): a column's counted rows from t = T - 1 down to 0; the 64 columns of a group n / 64 by the tree x[j] += x[j + w],
 * w = 32 .. 1 (columns past N: 0); the groups in contiguous runs of ceil(groups / 256) per thread of one 256-thread workgroup, each run in order, and the same tree with
 * w = 128 .. 1.  Two calls on one input give the same bytes.  The group partials live in `workspace` (dm_amp_batch_rewards_workspace(T, N) bytes, the caller's,
 * 8-byte aligned like stats_out).
 * Refused: T < 1, N < 1, T * N > 2^31 - 1; a NULL logits / rewards_out / bounds / stats_out / workspace; valid without done; a task reward with task_reward_lerp
 * outside [0, 1] (NaN: the agent has none); a workspace that is too small or misaligned; no HIP device or a device_id it does not have.
 *
 * dm_amp_value_clip.  out[i] = fminf(fmaxf(values[i], lo), hi) for i < n, with lo = (float)((double)bounds[0] / (1.0 - discount)) and hi likewise from bounds[1], read
 * on the device: the expression of the DM_SCALAR_HEAD_VALUE head, so with finite bounds the result is bit-identical to that head evaluated with lo / hi set to the same
 * floats.  row_mask int32[n] (NULL: every row): a row whose flag is 0 gets `fill`.  out may alias values.  The Fail / Succ override stays dm_td_lambda_returns' rule.
 * A NaN bound does not clip on its side (fmaxf / fminf return their other operand); a NaN value comes out as lo (as hi where lo is NaN too).  The initial bounds
 * {+inf, -inf} give -inf for every row.
 * Refused: n < 1, a NULL values / bounds / out, discount outside [0, 1), no HIP device or a device_id it does not have. */
enum { DM_AMP_STAT_N = 0, DM_AMP_STAT_MEAN = 1, DM_AMP_STAT_STD = 2, DM_AMP_STAT_MIN = 3, DM_AMP_STAT_MAX = 4, DM_AMP_STATS_WORDS = 5 };
int64_t dm_amp_batch_rewards_workspace(int T, int N);  /* < 0: refused (dm_last_error) */
int dm_amp_batch_rewards(int device_id, int T, int N, const float* logits_dev, const float* task_reward_dev /* NULL: style reward only */,
                         const int32_t* done_dev, const int32_t* valid_dev /* NULL: all valid */, double reward_scale, double task_reward_lerp,
                         float* rewards_out, int32_t* mask_out /* NULL or [T, N] */, float* bounds_dev /* [2] in/out */, double* stats_out /* [DM_AMP_STATS_WORDS] */,
                         void* workspace, int64_t workspace_bytes, void* hip_stream);
int dm_amp_value_clip(int device_id, int n, const float* values_dev, const float* bounds_dev /* [2] */, double discount, const int32_t* row_mask_dev /* NULL or [n] */,
                      double fill, float* out_dev, void* hip_stream);

/* ---- the test-mode time-warp return of `--scene imitate_amp` for a batch of envs (deepmimic_amd/csrc/dm_time_warp.h, dm_device.h k_time_warp_sample,
 * deepmimic_amd/time_warp.py): cSceneImitateAMP::CalcRewardTimeWarp (scenes/SceneImitateAMP.cpp:174-207, 417-480; util/DynamicTimeWarper.cpp:114-140), what the
 * reference's learner logs as Test_Return for an AMP imitation policy.  Stateless like dm_replay_* and dm_episode_stats: the caller owns every byte, DEVICE pointers
 * only, no allocation, no host read and no synchronisation inside; a refused call launches nothing.
 *   samples   [N][2][capacity][3J] elements of the context's precision (dm_time_warp_dims: out[0] = bytes per element, 4 or 8; out[1] = 3J); [.][0] the simulated,
 *             [.][1] the kinematic character; a row is BuildTimeWarpData: (0, root height, 0) for joint 0, joint position - root position for the others
 *   count     int32[N], rows held per env;  overflow: one int32 word, set to 1 by an append that found no room (the reference throws there), never cleared here
 * capacity is cSceneImitateAMP::BuildTimeWarper's buffer size, ceil(query rate * max(time_lim_max, time_end_lim_max)) + 2.
 *
 * dm_time_warp_sample: on the ctx's stream, in front of the step launch (the sample is the state at ENTRY of a control step, cRLSceneSimChar::PreUpdate).  Env i with
 * restart_dev[i] != 0 (restart_dev NULL: every env) starts over: count = 0, then TWO identical rows (ResetTimeWarper adds one, the PreUpdate of the first update
 * behind a reset one more, NeedNewAction being true there); any other env appends one row.  An append at count == capacity writes nothing, leaves count and sets
 * *overflow_dev.  Nothing outside env i's block is written.  With a multi-clip dataset the kinematic side is env i's own clip.
 * Refused: a NULL ctx / samples / count / overflow; capacity < 2; a context whose scene has no kinematic character to sample.
 *
 * dm_time_warp_align: needs no ctx; asynchronous on hip_stream of device device_id.  Per env i with select_dev[i] != 0 (select_dev NULL: every env) and n = count[i]:
 *     cost(0, 0) = 0, the rest of row 0 and column 0 +inf, cost(a, b) = d(a, b) + min(cost(a-1, b-1), cost(a-1, b), cost(a, b-1)) for 1 <= a, b < n,
 *     d(a, b) = (sum over the dim / 3 points p, in order, of |sim_a[p] - kin_b[p]|) / (dim / 3)
 *     reward_out[i] = cost(n-1, n-1) + (capacity - n) * term_step_cost (one rounding to float), cost_out[i] = cost(n-1, n-1) (NULL: not wanted)
 * n == 1: cost 0; n == 0 or select_dev[i] == 0: reward 0 and cost 0.  Distances in the element type (f64 == 0: float, else double), table values in fp64, no
 * contraction, no atomics: two calls on the same inputs give the same bytes.  One wavefront per env; the kernel's shape is described in dm_time_warp.h.
 * Refused: n_envs < 1; a NULL samples / count / reward_out; capacity < 2; dim not a positive multiple of 3; samples not aligned to its element, cost_out not 8-byte
 * aligned; 8 capacity + 192 (dim | 1) sizeof(element) above 160 KB (the workgroup's LDS); no HIP device or a device_id it does not have. */
int dm_time_warp_dims(const dm_ctx* ctx, int32_t* out /* [2] */);
int dm_time_warp_sample(dm_ctx* ctx, void* samples_dev, int32_t* count_dev /* [N] in/out */, const int32_t* restart_dev /* NULL: all */, int capacity,
                        int32_t* overflow_dev);
int dm_time_warp_align(int device_id, int n_envs, int capacity, int dim, int f64, const void* samples_dev, const int32_t* count_dev,
                       const int32_t* select_dev /* NULL: all */, double term_step_cost, float* reward_out_dev /* [N] */, double* cost_out_dev /* NULL or [N] */,
                       void* hip_stream);

/* ---- Link states as device tensors and a reset selected by a device mask, for tasks written in torch (deepmimic_amd/csrc/dm_link_state.h, k_link_state and
 * k_env_reset_where of dm_device.h, deepmimic_amd/link_state.py).  Every pointer but the ctx is a DEVICE pointer; both calls are asynchronous on the ctx's stream, read
 * nothing back and synchronise nothing; a refused call launches nothing and names its reason through dm_last_error.
 *
 * dm_link_state_dims: out[5] = J, 22, 8, P, 13 (0 on a context without a free body) -- the row widths of the outputs below.
 *
 * dm_link_state: the forward kinematics of the env record as it stands, float32 whatever the context's precision; a NULL output is skipped.
 *   which     0: the simulated character (the env's pose and velocity); 1: the kinematic character (the env's clip -- its own in a multi-clip dataset -- sampled at the
 *             env's clip time, about the origin of the env's kin row)
 *   links_dev [N][J][22]: 0:3 link COM world position; 3:12 body world rotation, row-major (cKinTree::BodyWorldTrans); 12:15 COM linear velocity
 *             (cKinTree::CalcBodyPartVel); 15:18 angular velocity (cKinTree::CalcJointWorldAngularVel); 18:21 joint world position (cKinTree::CalcJointPos);
 *             21 in contact: 1.0 where bit j of the env's contact mask (flags column 1 of dm_get_state: the last substep) is set, else 0.0; 0 for which = 1
 *   env_dev   [N][8]: character COM (3) and COM velocity (3) as cRBDUtil::CalcCoM; the root heading (cKinTree::BuildOriginTrans rotates about y by its negative); 0
 *   pose_dev, vel_dev [N][P]: the pose and velocity the link state was computed from (which = 1: the sampled clip pose)
 *   obj_dev   [N][13]: the free body of dribble_amp (position, rotation w x y z, linear and angular velocity), the columns of dm_get_obj_state
 * Behind a DM_AUTO_RESET launch the rows of envs it reset describe the first state of the new episode, as `states` does.  No atomics: two calls give the same bytes.
 * Refused: a NULL ctx; which outside {0, 1}; which = 1 on a scene without motion frames; obj_dev on a context without a free body.
 *
 * dm_reset_where: the start of a new episode for every env with mask_dev[i] != 0 (int32[N]), exactly what a DM_AUTO_RESET launch does for an env whose episode ended,
 * behind its outputs: every draw is the device's, keyed by the env's episode counter; RecordState of the new episode goes to row i of states_dev [N][S], RecordGoal
 * (goal scenes) to row i of goals_dev [N][dm_goal_size()] (may be NULL) and of the table dm_last_goals / dm_last_goals_device read.  No reward, flag or AMP row is
 * written.  Rows of unselected envs keep their bytes, in the context and in the outputs.  A control step launched without DM_AUTO_RESET (and with
 * DM_END_EPISODE_EARLY), then dm_reset_where of the envs that ended, leaves the context and `states` as the DM_AUTO_RESET launch leaves them -- with the end-of-step
 * state of every env, finished ones included, visible in between (tests/test_reset_where.py).
 * Refused: a NULL ctx, mask_dev or states_dev; goals_dev on a scene without a goal; a context with a draw tape bound (dm_set_draw_tape: that route draws on the host). */
int dm_link_state_dims(const dm_ctx* ctx, int32_t* out /* [5] */);
int dm_link_state(dm_ctx* ctx, int which, float* links_dev, float* env_dev, float* pose_dev, float* vel_dev, float* obj_dev);
int dm_reset_where(dm_ctx* ctx, const int32_t* mask_dev, float* states_dev, float* goals_dev);

/* ---- The kinematic character at times the caller chooses, and a masked reset whose clip, clip time and yaw the caller may give (deepmimic_amd/csrc/dm_kin_query.h,
 * k_kin_query and k_env_reset_where_at of dm_device.h, deepmimic_amd/kin_query.py).  As above: every pointer but the ctx is a DEVICE pointer, both calls are asynchronous
 * on the ctx's stream, read nothing back and synchronise nothing; a refused call launches nothing and names its reason through dm_last_error.
 *
 * dm_kin_query: K frames of the kinematic character per env, float32 whatever the context's precision; a NULL output is skipped.  The columns are those of
 * dm_link_state(which = 1) (dm_link_state_dims), the contact column is 0:
 *   links_dev [N][K][J][22], env_dev [N][K][8], pose_dev, vel_dev [N][K][P]
 *   times_dev float64 [K], shared by all envs, or [N][K] with DM_KIN_TIMES_PER_ENV.  A time is an offset added to the env's clip clock (negative offsets are allowed);
 *             with DM_KIN_TIMES_ABSOLUTE it is a clip time.
 *   clips_dev int32 [N], only with DM_KIN_TIMES_ABSOLUTE: the clip of the dataset to sample; NULL: the env's own clip, as dm_link_state picks it
 *   DM_KIN_ORIGIN_IDENTITY: about the identity origin instead of the origin of the env's kin row -- the clip in its own frame
 * A frame is cKinCharacter::CalcPose(t) / CalcVel(t) of the chosen clip about the chosen origin, then the forward kinematics of dm_link_state: a looping clip adds
 * cycle x cycle_delta to the root, a clip that does not loop clamps to its first / last frame and its velocity is 0 from its end on.  The root sync a phase wrap of the
 * env's clock applies (SyncKinCharNewCycle) is not anticipated.  An offset of 0 gives the bytes of dm_link_state(which = 1).  A non-finite time, or a clip id outside
 * [0, num_clips), makes every output row of that (env, k) NaN; no table is indexed with either.  No atomics: two calls give the same bytes.
 * Refused: a NULL ctx or times_dev; K outside [1, 64]; a scene without motion frames; clips_dev without DM_KIN_TIMES_ABSOLUTE; unknown flag bits.
 *
 * dm_reset_where_at: dm_reset_where for every env with mask_dev[i] != 0, where each of clip, clip time and yaw is given or drawn per env: clips_dev[i] >= 0 gives
 * the clip (-1 or a NULL array: drawn), a finite times_dev[i] the clip time (NaN or NULL: drawn), a finite yaw_dev[i] the yaw about +y (NaN or NULL: the rule below).
 *   nothing given:  exactly dm_reset_where, recovery episodes of a get-up scene included
 *   anything given: a full scene reset without a recovery episode (the rule dm_reset applies to a given kin_time).  The time limit is drawn as always (stream 1); a
 *                   clip that is not given by weight (stream 3); a time that is not given uniformly over the duration of the clip the episode starts on (stream 0);
 *                   a yaw that is not given is 0 when the time is given, else the scene's rule (enable_rand_rot_reset, stream 4).  A given yaw applies in a plain
 *                   scene too.  clips = 0 and a time, nothing else: the context and the rows are those of dm_reset(ids, kin_times).
 * Invalid: a clip id >= num_clips or < -1, a negative or infinite time, an infinite yaw.  Such an env keeps every byte of its state and of its output rows, and the
 * kernel stores 1 to bad_dev[0] (int32, may be NULL; the caller zeroes it before the call).
 * Refused: as dm_reset_where -- a NULL ctx, mask_dev or states_dev; goals_dev on a scene without a goal; a context with a draw tape bound. */
enum { DM_KIN_TIMES_PER_ENV = 1, DM_KIN_TIMES_ABSOLUTE = 2, DM_KIN_ORIGIN_IDENTITY = 4 };
int dm_kin_query(dm_ctx* ctx, int K, const double* times_dev, const int32_t* clips_dev /* NULL */, int flags, float* links_dev, float* env_dev, float* pose_dev,
                 float* vel_dev);
int dm_reset_where_at(dm_ctx* ctx, const int32_t* mask_dev, const int32_t* clips_dev, const double* times_dev, const double* yaw_dev, float* states_dev,
                      float* goals_dev, int32_t* bad_dev /* NULL */);

/* ---- A pool of whole env records in device memory: save the envs a device mask selects into slots of the pool, and start envs from slots -- a rewind, or a new
 * episode from a stored state (deepmimic_amd/csrc/dm_state_pool.h, k_state_save and k_state_restore of dm_device.h, deepmimic_amd/state_pool.py).  The pool is the
 * caller's device memory (16-byte aligned, dm_state_pool_bytes(ctx, slots) bytes), as with dm_replay_*; save and restore are asynchronous on the ctx's stream, read
 * nothing back and synchronise nothing; a refused call launches nothing and names its reason through dm_last_error.
 *
 * A slot is one env's record in the ctx's precision: the rows of the env the next control step or query depends on -- pose, vel, tar, tau, kin, clock, flag and,
 * where the ctx has them, hist (the AMP pose history), obj (the free body), goal, pert and manif (DM-physics v2) -- back to back in that order, every segment on a
 * 16-byte boundary, the slot a multiple of 16 bytes.  It holds no pointer and no env id: a pool copied elsewhere on the device, or to the host and back, restores
 * the same bytes.  dm_state_pool_dims: out[0] the slot size in bytes, out[1 .. 12] the byte offset of each segment in the order above (-1: the ctx has no such row).
 * Only contexts with equal dims may share a pool.
 *
 * dm_state_save: every env with mask_dev[i] != 0 writes its record into slot slots_dev[i] of pool_dev.  Two selected envs of one call that name the same slot break
 * the contract: that slot's content is then unspecified, nothing else is touched.
 * dm_state_restore: every env with mask_dev[i] != 0 takes the record of slot slots_dev[i]; many envs may name one slot.  Three things belong to the env and not to
 * its state and stay as the destination has them: the diagnostic counters ("fallback", "borrowed" of dm_get_debug), the env's own draw key in the goal row and in
 * the perturbation row (dm_set_env_keys).  Then, as dm_reset_where behind its reset, RecordState goes to row i of states_dev (may be NULL) and RecordGoal to the
 * ctx's last-goals row and to row i of goals_dev (may be NULL); no reward, flag or AMP row is written.  flags:
 *   DM_POOL_REWIND       the record as stored, the pose history included.  The same actions then reproduce the stored env's rollout bit for bit on the env that saved
 *                        it; on another env of the ctx everything that is not a draw reproduces too.
 *   DM_POOL_NEW_EPISODE  a new episode that starts at the stored state: the destination keeps its episode counter, advanced by one as a reset advances it, and its
 *                        goal and perturbation draw counters, so that the draws behind the start do not repeat whenever a slot is used; the episode timer starts
 *                        over (time 0, the limit drawn with the new counter as every reset draws it); the pose history is re-initialised as a reset does; valid is
 *                        1 and the contact latch is cleared.  Pose, velocity, targets, latched torque, kin origin, the kin and control clocks, clip, goal target and
 *                        goal timers, the free body, active perturbation forces and manifolds are the slot's.
 * A selected env whose slot is outside [0, slots) keeps every byte of its state (a save writes nothing), and the kernel stores 1 to bad_dev[0] (int32, may be NULL;
 * the caller zeroes it before the call).
 * Refused: a NULL ctx, pool_dev, mask_dev or slots_dev; a pool that is not 16-byte aligned; slots <= 0; unknown flag bits; goals_dev on a scene without a goal; a
 * context with a draw tape bound.  dm_state_pool_bytes returns a negative value when it refuses. */
enum { DM_POOL_REWIND = 0, DM_POOL_NEW_EPISODE = 1 };
int64_t dm_state_pool_bytes(const dm_ctx* ctx, int slots);
int dm_state_pool_dims(const dm_ctx* ctx, int32_t* out /* [13] */);
int dm_state_save(dm_ctx* ctx, void* pool_dev, int slots, const int32_t* mask_dev, const int32_t* slots_dev, int32_t* bad_dev /* NULL */);
int dm_state_restore(dm_ctx* ctx, const void* pool_dev, int slots, const int32_t* mask_dev, const int32_t* slots_dev, int flags, float* states_dev /* NULL */,
                     float* goals_dev /* NULL */, int32_t* bad_dev /* NULL */);

/* ---- Task-chosen pushes: place forces on body parts from device tensors, and read out the forces that are acting (deepmimic_amd/csrc/dm_push.h, k_push_where and
 * k_push_state of dm_device.h, deepmimic_amd/pushes.py).  The forces live in the two slots of the env's perturbation row (dm_get_perturb_state) and are applied by the
 * step kernels exactly as a drawn perturbation is: at the body part's centre of mass, for whole scene updates.  The ctx needs the rows: enable_rand_perturbs, where
 * an infinite interval gives rows without the random schedule (dm_scene_tables).  With the random schedule on, both share the two slots.  Every pointer but the ctx
 * is a device pointer; both calls are asynchronous on the ctx's stream, read nothing back and synchronise nothing; a refused call launches nothing and names its
 * reason through dm_last_error.
 *
 * dm_push_where: for every env with mask_dev[i] != 0, the force forces_dev[i] (N x 3 doubles, newtons) acts on body part links_dev[i] for durations_dev[i]
 * seconds: from the first scene update of the next launch, for whole updates while elapsed < duration -- ceil(duration / dt) updates, across control steps; a zero
 * duration never acts, +infinity lasts until the episode's reset clears it (every scene reset clears both slots; dm_state_restore brings the forces stored in a
 * slot of the pool).  slots_dev[i] 0 or 1 names the slot of the row; -1, or a NULL array, takes the rule of a drawn force: a free slot, lowest index first, else
 * the slot nearest its end (the largest elapsed - duration), whose force is replaced.  links_dev[i] == -1 frees the named slot, or both for slot -1.
 * flags: DM_PUSH_WORLD, the force is in world coordinates and stored as given; DM_PUSH_HEADING, it is given in the character's heading frame (x forward, y up,
 * the frame of dm_link_state's heading column) and stored as rot_y(heading of the root rotation) * f, computed in the ctx's precision at the time of the call:
 * a fixed world direction afterwards.  The row's clock, next time, draw counter and draw key are not touched and no draw is made.  Two calls with the same
 * arguments leave the same bytes.
 * A selected env with a link outside [-1, num_joints), a non-finite force component, a negative or NaN duration, or a slot outside [-1, 2) keeps every byte, and
 * the kernel stores 1 to bad_dev[0] (int32, may be NULL; the caller zeroes it before the call); the other envs of the call are served.
 * Refused: a NULL ctx, mask_dev, links_dev, forces_dev or durations_dev; unknown flag bits; a ctx without perturbation rows.
 *
 * dm_push_state: out_dev [N][2][6] float32 whatever the precision: per slot {link (-1: free, the other columns are 0 then), fx, fy, fz, duration, elapsed}.  A
 * force whose time is up leaves its slot at the next scene update. */
enum { DM_PUSH_WORLD = 0, DM_PUSH_HEADING = 1 };
int dm_push_where(dm_ctx* ctx, const int32_t* mask_dev, const int32_t* links_dev, const double* forces_dev /* [N][3] */, const double* durations_dev,
                  const int32_t* slots_dev /* NULL */, int flags, int32_t* bad_dev /* NULL */);
int dm_push_state(dm_ctx* ctx, float* out_dev /* [N][2][6] */);

/* ---- PPO actor and critic minibatch updates on the device (deepmimic_amd/csrc/dm_train.h, deepmimic_amd/train.py): PPOAgent._update_actor / _update_critic and
 * MPISolver.update (learning/ppo_agent.py:95-139, 286-309, learning/solvers/mpi_solver.py:33-54) for the plain three-layer nets, on the context that samples, so that
 * exp(logp_new - logp_old) is 1 (to rounding) at the weights that sampled.  Stateless like dm_ppo_*, dm_replay_* and dm_episode_stats: the caller owns every byte, all
 * pointers are DEVICE pointers, calls are asynchronous on hip_stream, nothing is read on the host or synchronised inside, a refused call launches nothing, writes nothing
 * and names its reason through dm_last_error.  The one object is the dm_policy whose net is trained: its packed bf16 weights and its activation buffers s16 / h1 / h2 are
 * read and written; the buffers grow to the largest n as in dm_policy_forward_ex (the one allocation).  ORDERING: like dm_policy_set_weights, a training call must not
 * run while another stream runs a forward, a scalar evaluation, a refresh or another training call of the same context -- order them with events or use one stream.
 * Out of scope: one fused training kernel (Adam, gradient clipping and the non-finite guard: dm_train_opt_step below; a step-size schedule is the caller passing
 * another step size, an argument of every step).  The AMP discriminator update is dm_train_disc_grad below; gated
 * contexts have entry points of their own, dm_train_gated_* further below, and these calls refuse them.
 *
 * Parameter block: P = dm_train_param_count(net) floats in the order w1 [S x H1], b1, w2 [H1 x H2], b2, w3 [H2 x A], b3; matrices in tf.layers.dense layout (in x out,
 * row-major), true widths, no padding.  The caller holds three such arrays: masters, momentum, gradients.
 * PRECONDITION of the two *_grad calls: the net's packed weights are the round-to-nearest-even bf16 of params_dev (the backward pass multiplies by the bf16 of the
 * masters, the forward pass by the packed arrays).  dm_train_sgd_step with the net keeps this true; dm_policy_set_weights from the block establishes it.
 *
 * Arithmetic (the specification; deepmimic_amd/train.py reference_grad / reference_step state it in numpy):
 *   forward   k_policy_prep and layers 1 and 2 on the context's per-layer kernels as the widths choose them, whatever DM_POLICY_* says, with the bound observation
 *             normaliser: s16, h1, h2 in bf16; z3 = h2 w3 + b3 with fp32 accumulation of bf16 products (the chain of the sampling net's layer 3).  logstd is not trained
 *             (StdType.Default).
 *   actor     per row i, all in fp32 with one rounding per written operation: x = (a - a_mean) / a_std, sigma = exp(logstd), mu = z3, u_j = (x_j - mu_j) / sigma_j,
 *             logp = fmaf(-0.5, sum_j u_j^2, (-0.5 A) ln 2pi - sum_j logstd_j), ratio = exp(logp - old_logp), l0 = adv ratio, l1 = adv clip(ratio, 1 - eps, 1 + eps),
 *             g_i = -(l0 / n) unless l0 > l1, else 0 (tf.minimum sends the gradient of a tie to its first argument),
 *             dz3_ij = fmaf(bound_weight / n, min(mu_j - lo_j, 0) + max(mu_j - hi_j, 0), g_i (u_j / sigma_j)), lo / hi = (bound - a_mean) / a_std (learning/pg_agent.py:189-202,
 *             tf_util.py:65-81).  exp is the library's own (dm_train.h exp_det: every rounding point written down, within 2 ulp), the row sums run over each lane's
 *             columns c, 16 + c, .. ascending and then a pairwise tree over c.
 *   critic    dz3_i = (v_i - tar_i) / n; no value clip, as in the reference's training graph.
 *   stats     fp64 sums in a fixed order (per 16 rows in row order, the blocks by contiguous runs and a fixed tree), no atomics: two calls on one input are bit-identical.
 *   backward  every matrix-core operand bf16 (RNE), accumulation fp32, gradients fp32: dW_l = in_l^T dz_l with in_l the saved bf16 activation (s16 without its padding
 *             columns, h1, h2) and dz_l rounded to bf16; db_l = the column sums of the same bf16 dz_l in fp32 (four contiguous row quarters, each ascending, added in order); dz_(l-1) = (dz_l W_l^T) . [h_(l-1) != 0]
 *             with W_l the RNE bf16 of the masters.  The contraction over the rows is not split: no partials, no floating-point atomics.
 *   A non-finite action, advantage, old logp, target or master gives non-finite gradients; nothing clamps.  (Observations pass the normaliser's clip as for the
 *   sampling net: a NaN observation becomes -s_clip there.)
 *   step      (tf.train.MomentumOptimizer behind MPISolver) per element: g = grad_scale grad, on matrix entries g += weight_decay w (_weight_decay_loss skips
 *             biases), v = momentum v + g -- these in fp64, where every product of two floats is exact, v rounded to fp32 ONCE (a chain of fp32 roundings is off by
 *             many ulps of a v that momentum v and g nearly cancel to); then w = fmaf(-stepsize, v, w) with the stored v.  Device and emulator round alike.
 *             With a net the new masters are then packed into it: dm_policy_set_weights with
 *             DM_DEVICE_PTRS on views of params_dev, byte for byte what dm_policy_create makes of the same arrays.  Without one (NULL) only the step runs, on the
 *             current device, and weight_decay must be 0 (which entries are matrices is the net's layout).
 *
 * Workspace (dm_train_workspace_bytes(net, n) bytes, 16-byte aligned), left behind by a *_grad call:
 *   [z3 fp32 n x N3][dz3 bf16 n x N3][dz2 bf16 n x H2][dz1 bf16 n x H1][ceil(n / 16) blocks of 8 doubles], N3 = action_dim rounded up to 32, padded columns zero.
 * dm_train_actor_grad: cfg->a_bound_min / a_bound_max are HOST arrays of action_dim un-normalised entries (+-inf allowed; both NULL: no bound loss), bound_weight is 10
 *   in the reference.  grads_dev [P] is overwritten; stats_dev double[6] = {n, -mean min(l0, l1), bound loss 0.5 mean sum_j violation^2, clip_frac = mean[|ratio - 1| > eps],
 *   mean ratio, mean logp_new}; logp_out [n] optional.
 * dm_train_value_grad: stats_dev double[2] = {0.5 mean (tar - v)^2, mean v}; values_out [n] optional, the raw net output.
 * Refused: a NULL net or required pointer; a gated context; n < 1; a workspace that is too small or not 16-byte aligned, stats not 8-byte aligned; a goal_dim
 * dm_policy_forward_ex would refuse; ratio_clip <= 0; bound_weight < 0; one of the two bound arrays without the other; the actor call on a context without logstd /
 * a_mean / a_std or with action_dim > 128; the value call on action_dim != 1; stepsize, momentum or weight_decay negative or non-finite, a non-finite grad_scale;
 * P < 1 or, with a net, P != dm_train_param_count(net); weight_decay != 0 without a net.
 * dm_train_read_activations: TEST SUPPORT, synchronous: the first n rows of s16 [n x K1] (which = 0), h1 (1) or h2 (2) as the last call left them, bf16, to the host. */
typedef struct dm_train_actor_cfg { double ratio_clip, bound_weight; const float* a_bound_min; const float* a_bound_max; } dm_train_actor_cfg;
int64_t dm_train_param_count(const dm_policy* net);                 /* < 0: refused (dm_last_error) */
int64_t dm_train_workspace_bytes(const dm_policy* net, int n);      /* < 0: refused (dm_last_error) */
int dm_train_actor_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* actions_dev,
                        const float* old_logp_dev, const float* adv_dev, const dm_train_actor_cfg* cfg, float* grads_dev, double* stats_dev, float* logp_out,
                        void* workspace, int64_t workspace_bytes, void* hip_stream);
int dm_train_value_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* targets_dev,
                        float* grads_dev, double* stats_dev, float* values_out, void* workspace, int64_t workspace_bytes, void* hip_stream);
int dm_train_sgd_step(dm_policy* net, float* params_dev, float* momentum_dev, const float* grads_dev, int64_t P, double stepsize, double momentum,
                      double weight_decay, double grad_scale, void* hip_stream);
int dm_train_read_activations(dm_policy* net, int which, int n, void* host_out, size_t capacity);

/* ---- The AMP discriminator minibatch update, gradient penalty included (deepmimic_amd/csrc/dm_train.h, deepmimic_amd/train.py DiscTrainer): AMPAgent._step_disc
 * (learning/amp_agent.py:134-207, 251-257, 356-377) on the context that scores the style reward (dm_policy_eval_scalar), under the rules of the section above: stateless,
 * DEVICE pointers, asynchronous on hip_stream, a refused call launches and writes nothing, the PRECONDITION on the packed weights, the parameter block, dm_train_sgd_step
 * (which carries DiscWeightDecay) and dm_train_read_activations unchanged.  The net is plain (not gated), action_dim = 1, no goal block.
 *
 * The two batches are separate arrays [n_expert x S] and [n_agent x S], what dm_amp_expert_draw / dm_replay_sample fill; in every per-row output (activations, workspace,
 * logits_out) the expert rows come first.  x is the normalised, clipped bf16 observation, h1 / h2 the bf16 ReLU activations, m_k = [h_k != 0], y = h2 w3 + b3,
 * c_gp = cfg->grad_penalty (DiscGradPenalty), c_lr = cfg->logit_reg (DiscLogitRegWeight):
 *   loss = 0.5 (mean_e 0.5 (y - 1)^2 + mean_a 0.5 (y + 1)^2) + c_gp 0.5 mean_e |dy/dx|^2 + c_lr 0.5 |w3|^2       (the penalty on the normalised input, expert rows only)
 * Arithmetic (deepmimic_amd/train.py reference_disc_head / reference_disc_grad state it in numpy):
 *   forward   as in the section above; y is the chain of the scalar head (column tile 0, k-steps ascending from zero) plus b3: the bits dm_policy_eval_scalar's per-layer route gives.
 *   head      fp32, one rounding per written operation: e = y - t with t = +1 (expert) / -1 (agent), dz3 = bf16((0.5 e) / n_side) with n_side = n_expert or n_agent as float.
 *   least squares   the backward pass of the section above over all n_expert + n_agent rows from that dz3: every gradient element WRITTEN.
 *   penalty   (c_gp > 0; expert rows) every operand bf16, accumulation fp32, k-steps ascending from a ZERO accumulator, results rounded to bf16 (RNE) where stored:
 *             g2 = bf16(w3) . m2;  g1 = bf16((g2 W2^T) . m1);  gx = g1 W1^T in fp32, not stored;  per row and per block of 32 columns sq = the lane sums v0 v0 then
 *             fmaf(v1, v1, .) over its columns c, 16 + c, then a pairwise tree over c (fp32);  a = bf16(gx (float(c_gp) / float(n_expert))), padding columns zero;
 *             t1 = bf16((a W1) . m1);  t2 = bf16((t1 W2) . m2), both on the PACKED bf16 weights (= RNE bf16 of the masters by the precondition).
 *   ROUNDING ORDER of a gradient element, by its one owner (no atomics, no split contraction): the least-squares value (its own contraction, rounded to fp32, stored);
 *             then, c_gp > 0 only, the penalty value (its own contraction: dW1 a^T g1, dW2 t1^T g2, dw3 the column sums of t2 as dm_train's db) is ADDED by one fp32 add:
 *             dW = fl(ls + pen); then, c_lr > 0 only, the regulariser by one fmaf on the fp32 master: dw3 = fmaf(float(c_lr), w3, dw3).  The biases get the
 *             least-squares value alone.  c_gp = 0 skips the whole penalty path (its statistic is 0); c_gp = c_lr = 0 and n_expert = n_agent is, bit for bit,
 *             dm_train_value_grad on the concatenated rows with targets +-1.
 *   stats_dev double[8] = {least-squares loss, acc_expert = mean_e [y > 0], acc_agent = mean_a [y < 0], mean_a sigmoid(y) (fp32 1 / (1 + exp_det(-y))), mean_a |y|,
 *             gradient penalty 0.5 mean_e sum sq, 0.5 |w3|^2, 0.5 sum_k |W_k|^2 over the three matrix masters}: fp64 sums in a fixed order (per 16 rows in row order, then
 *             contiguous runs per thread and a fixed tree).  The reference's Disc_Loss is stats[0] + c_gp stats[5] + c_lr stats[6] + DiscWeightDecay stats[7].
 * Workspace (dm_train_disc_workspace_bytes, 16-byte aligned), left behind: the five pieces of the section above for n = n_expert + n_agent rows, then
 *   [g2 bf16 n_e x H2][g1 bf16 n_e x H1][a bf16 n_e x K1][t1 bf16 n_e x H1][t2 bf16 n_e x H2][sq fp32 n_e x K1 / 32, padded to 16 bytes][128 doubles: weight-norm partials].
 *   With c_gp = 0 the pieces from g2 to sq are not written.
 * Refused: a NULL net or required pointer (logits_out [n_expert + n_agent] is optional); a gated context; action_dim != 1; n_expert < 1 or n_agent < 1; grad_penalty or
 * logit_reg negative or non-finite; a workspace that is too small or not 16-byte aligned, stats not 8-byte aligned; (n_expert + n_agent) max(K1, H1, H2) >= 2^31. */
typedef struct dm_train_disc_cfg { double grad_penalty, logit_reg; } dm_train_disc_cfg;
int64_t dm_train_disc_workspace_bytes(const dm_policy* net, int n_expert, int n_agent);      /* < 0: refused (dm_last_error) */
int dm_train_disc_grad(dm_policy* net, const float* params_dev, const float* expert_obs_dev, int n_expert, const float* agent_obs_dev, int n_agent,
                       const dm_train_disc_cfg* cfg, float* grads_dev, double* stats_dev, float* logits_out, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- The PPO actor and critic minibatch updates for GATED contexts (deepmimic_amd/csrc/dm_train_gated.h, deepmimic_amd/train.py GatedActorTrainer / GatedCriticTrainer):
 * the nets of the AMP task agents (ct_agent_humanoid_amp_tasks*.txt: "ActorNet" and "CriticNet" fc_2layers_gated_1024units), trained on the context that samples
 * (dm_policy_create_gated).  New entry points beside the dm_train_* of the plain nets, which keep refusing a gated context; the rules of that section hold: stateless, DEVICE
 * pointers, asynchronous on hip_stream, nothing allocated beyond the context's activation buffers, a refused call launches and writes nothing and names its reason, the
 * ORDERING rule, the PRECONDITION (the packed weights of all twenty arrays are the RNE bf16 of params_dev; dm_train_gated_sgd_step keeps it true, dm_policy_set_weights with
 * the gate struct from the block establishes it), the actor and critic heads, the statistics and dm_train_actor_cfg unchanged.
 *
 * Notation (dm_policy_gate_params; i = 0: layer 1, width H1; i = 1: layer 2, width H2; GC = gate_common, GH = gate_hidden, G = goal_dim, KG = G rounded up to 32):
 *   xg = the bf16 goal block of s16;  c = relu(Wc xg + bc);  e_i = relu(We_i c + be_i);  beta_i = Wb_i e_i + bb_i;  sigma_i = 2 sigmoid(Ws_i e_i + bs_i);
 *   u_i = W_i h_(i-1) + b_i;  p_i = fmaf(sigma_i, u_i, beta_i);  h_i = bf16(relu(p_i)).
 * Arithmetic (the specification; deepmimic_amd/train.py reference_gated_grad states it in numpy):
 *   forward   the context's per-layer gated route, forced: k_policy_prep, k_policy_gate, the GATED layer kernels as the widths choose them: s16, h1, h2 in bf16 and
 *             sigma_i, beta_i in fp32 with the rounding points of dm_policy.h GateDev.  xg [n x KG] (padding columns zero), c [n x GC], e_0, e_1 [n x GH] are formed once
 *             more by the function the forward uses (dmp::gate_hidden: the same bits) and written to the workspace as row-major bf16.
 *   head, statistics, layer 3   as in the plain section: dW3 = h2^T dz3, db3, dp_1 = bf16((dz3 W3^T) . [h2 != 0]).
 *   gate split   once per hidden layer, i = 1 then 0.  acc is recomputed by the forward's chain (packed bf16 fragments, k-steps ascending from a zero accumulator), u = acc + b.
 *             Per element in fp32, one rounding per written operation, dp the bf16 value: du = bf16(dp sigma);  t = fmaf(-0.5, sigma, 1), ds = sigma t (dsigma/dz of
 *             sigma = 2 sigmoid(z));  da = bf16((dp u) ds).  The ReLU mask [h != 0] is already inside dp.  sigma = 0 and sigma = 2 give ds = 0; a NaN propagates.
 *   main layers  as in the plain section from du_i in dz_i's place: dW_i = in^T du_i, db_i = the column sums of du_i, dp_0 = bf16((du_1 W2^T) . [h1 != 0]).
 *   gate projections   dWb_i = e_i^T dp_i, dbb_i = the column sums of dp_i;  dWs_i = e_i^T da_i, dbs_i = the column sums of da_i.
 *   gate hidden layers   dze_i = bf16((dp_i Wb_i^T + da_i Ws_i^T) . [e_i != 0]): ONE accumulator started at zero, the k-steps of the beta pair ascending, then those of the
 *             sigma pair; B operands the RNE bf16 of the masters.  dWe_i = c^T dze_i, dbe_i its column sums.  dzc = bf16((dze_0 We_0^T + dze_1 We_1^T) . [c != 0]) the same
 *             way, pair 0 first.  dWc = xg^T dzc over the true G rows, dbc its column sums.  Nothing flows into the observations.
 *   Every gradient element is written by its one owner from one contraction: no split contraction, no atomic, no partial; two calls on one input give the same bytes, in
 *   the workspace as well.
 *   step      k_train_sgd's arithmetic per element; the weight decay falls on all TEN matrices and on none of the ten vectors (_weight_decay_loss drops only variables
 *             whose name contains "bias"; gate{i}/dense/kernel, the beta projection, is not one).  Then the context is refreshed from the new masters, gate included
 *             (dm_policy_set_weights with both structs and DM_DEVICE_PTRS on views of params_dev).
 * Parameter block: P = dm_train_gated_param_count(net) floats: the six arrays of the plain block, then the gate's in the order of dm_policy_gate_params -- gc_w [G x GC],
 *   gc_b, g0_w [GC x GH], g0_b, g0_bias_w [GH x H1], g0_bias_b, g0_scale_w, g0_scale_b, then g1_* with H2 -- tf.layers.dense layout, true widths, no padding.
 * Workspace (dm_train_gated_workspace_bytes(net, n), 16-byte aligned), left behind: the five pieces of the plain section, its dz2 / dz1 slots holding dp_1 / dp_0, then, all
 *   bf16 and each piece starting on a multiple of 16 bytes,
 *   [du_1 n x H2][du_0 n x H1][da_1 n x H2][da_0 n x H1][xg n x KG][c n x GC][e_0 n x GH][e_1 n x GH][dze_0 n x GH][dze_1 n x GH][dzc n x GC].
 * Refused: a NULL net; a PLAIN context (dm_policy_create: "a plain context"); everything the plain calls refuse in the same words; a goal_dim other than 0 or the gate's;
 * in the step P != dm_train_gated_param_count(net).  dm_train_gated_sgd_step needs its net.
 * dm_train_gated_read: TEST SUPPORT, synchronous: the first n rows of s16 (which = 0), h1 (1), h2 (2) in bf16 or of sigma_0 (3), beta_0 (4) [n x H1], sigma_1 (5),
 * beta_1 (6) [n x H2] in fp32, as the last call left them, to the host. */
int64_t dm_train_gated_param_count(const dm_policy* net);                 /* < 0: refused (dm_last_error) */
int64_t dm_train_gated_workspace_bytes(const dm_policy* net, int n);      /* < 0: refused (dm_last_error) */
int dm_train_gated_actor_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* actions_dev,
                              const float* old_logp_dev, const float* adv_dev, const dm_train_actor_cfg* cfg, float* grads_dev, double* stats_dev, float* logp_out,
                              void* workspace, int64_t workspace_bytes, void* hip_stream);
int dm_train_gated_value_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* targets_dev,
                              float* grads_dev, double* stats_dev, float* values_out, void* workspace, int64_t workspace_bytes, void* hip_stream);
int dm_train_gated_sgd_step(dm_policy* net, float* params_dev, float* momentum_dev, const float* grads_dev, int64_t P, double stepsize, double momentum,
                            double weight_decay, double grad_scale, void* hip_stream);
int dm_train_gated_read(dm_policy* net, int which, int n, void* host_out, size_t capacity);

/* ---- Adam, global-norm gradient clipping and a non-finite guard for the device trainers (deepmimic_amd/csrc/dm_optim.h, deepmimic_amd/train.py): ONE optimiser step for
 * plain, gated and discriminator contexts beside dm_train_sgd_step / dm_train_gated_sgd_step, which stay as they are.  The rules of the sections above hold: DEVICE
 * pointers, asynchronous on hip_stream, nothing read on the host or synchronised, a refused call launches and writes nothing and names its reason, the ORDERING rule.  With
 * a net (plain: the block of dm_train_param_count, weight decay on its three matrices; gated: dm_train_gated_param_count, on its ten) the context is refreshed from the
 * masters as those steps refresh it, gate included, after a skipped step too (the same bytes again); net NULL: the step alone on the current device, weight_decay 0.
 *
 * cfg: kind DM_OPT_MOMENTUM (beta1 is the momentum; beta2 and eps are not used, v_dev may be NULL) or DM_OPT_ADAM; max_grad_norm <= 0 or +inf: no clipping;
 * skip_nonfinite != 0: the guard.  Below B1 = (double)(float)beta1, likewise B2, wd, eps; stepsize, grad_scale and max_grad_norm enter as the doubles they are.
 * state_dev double[8], the caller's, ZERO before the first step, a checkpoint together with the arrays:
 *   [0] t, the steps taken (an exact integer)   [1] B1^t   [2] B2^t (running fp64 products; t = 0 reads both as 1 whatever the words hold)   [3] the steps skipped
 *   [4] the last norm   [5] the last scale   [6] the last number of non-finite gradient elements   [7] reserved
 * Arithmetic (the specification; reference_grad_norm / reference_opt_begin / reference_adam_step / reference_step of deepmimic_amd/train.py state it in numpy), every
 * written operation rounded once in fp64, no product contracted into a sum:
 *   norm pass  only with clipping or the guard.  Group b of G = ceil(P / 1024) owns the elements from 1024 b; its thread t adds g_i^2 (exact in fp64) for
 *              i = 1024 b + t + 256 k, k = 0 .. 3, in that order and counts its elements that are NaN or +-inf; the 256 threads by the tree x[t] += x[t + w],
 *              w = 128 .. 1; the G partials by contiguous runs of ceil(G / 256) per thread, each in order, and the same tree.  Two calls give the same bytes.
 *   decisions  norm = |grad_scale| sqrt(sum);  scale = min(1, max_grad_norm / (norm + 1e-6)) with clipping (torch.nn.utils.clip_grad_norm_'s rule; a NaN quotient
 *              stays NaN, as np.minimum keeps it), else 1;  skip = guard and count > 0.  Without the norm pass sum = count = 0 and words 4 and 6 are written as 0.
 *              Unless skip: t += 1, and the two powers are multiplied by B1 and B2 (MOMENTUM keeps them alike; B2 feeds nothing else there).  With skip: word 3 += 1,
 *              words 0 to 2 and every array keep their bytes.  s = (float)(grad_scale scale);  ADAM: alpha_t = stepsize / (1 - B1^t), ic2 = 1 / (1 - B2^t).
 *   step       per element g = (double)s (double)grad; on matrix entries g += wd w (L2 added to the gradient, as the momentum step and torch.optim.Adam do it; biases
 *              exempt).  MOMENTUM: the step of dm_train_sgd_step with s in place of (float)grad_scale -- with no clipping and no guard the same bytes.
 *              ADAM: m' = (float)(B1 m + (1 - B1) g);  v' = (float)(B2 v + ((1 - B2) g) g);  w' = (float)(w - (alpha_t m') / (sqrt(v' ic2) + eps)) with the stored
 *              m' and v'; sqrt and the division correctly rounded.  Device and emulator round alike.
 *   A non-finite gradient element with the guard off spreads as this arithmetic says: an infinite norm gives scale 0 and 0 inf = NaN in that element, a NaN norm
 *   gives s = NaN and every element NaN.
 * Workspace (dm_train_opt_workspace_bytes(P) = 32 + 16 G bytes, 16-byte aligned), left behind: [control record {int32 skip, float s, double alpha_t, double ic2}, padded
 *   to 32 bytes][G doubles: the groups' sums][G doubles: their counts].
 * Refused: a NULL cfg, params, m, grads, state or workspace; an unknown kind; ADAM without v_dev, with (float)beta1 or (float)beta2 outside [0, 1) or (float)eps not
 * finite and > 0; MOMENTUM with a negative or non-finite beta1; stepsize or weight_decay negative or non-finite; a non-finite grad_scale; a NaN max_grad_norm; P < 1
 * or > 2^40 or, with a net, P != its parameter count; weight_decay != 0 without a net; a state that is not 8-byte aligned; a workspace that is too small or not
 * 16-byte aligned. */
enum { DM_OPT_MOMENTUM = 0, DM_OPT_ADAM = 1 };
typedef struct dm_train_opt_cfg {
    int32_t kind, skip_nonfinite;
    double stepsize, beta1 /* MOMENTUM: the momentum */, beta2, eps, weight_decay, grad_scale;
    double max_grad_norm;            /* <= 0 or +inf: no clipping */
} dm_train_opt_cfg;
int64_t dm_train_opt_workspace_bytes(int64_t P);      /* < 0: refused (dm_last_error) */
int dm_train_opt_step(dm_policy* net /* NULL: the step alone, weight_decay must be 0 */, const dm_train_opt_cfg* cfg, float* params_dev, float* m_dev,
                      float* v_dev /* ADAM only, else NULL */, const float* grads_dev, int64_t P,
                      double* state_dev /* [8], 8-byte aligned, caller-owned, zero before the first step */, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- a probe for the device math helpers(deepmimic_amd/csrc/dm_math.h, dm_math_probe.h): TEST SUPPORT, nothing of the product calls it.  One launch evaluates the
 * helper `op` on n independent rows, one lane per row: row i reads in_dev[i * DM_MATH_PROBE_IN ..] and writes out_dev[i * DM_MATH_PROBE_OUT ..], doubles both, DEVICE
 * pointers.  The kernel narrows the inputs the op reads to float (f64 == 0) or keeps them double (f64 != 0), calls the helper in that type, and widens the result
 * (exact); outputs the op does not produce are written as 0, rows >= n are not touched.  Quaternions are (w, x, y, z), matrices row-major.
 *     op                       reads                                                    writes
 *     SINCOS                   x = in[0]                                                sin, cos
 *     ROT_Y, ROT_Z             angle = in[0]                                            3 x 3
 *     NORMALIZE_ANGLE          angle = in[0]                                            angle
 *     QMUL                     a = in[0..3], b = in[4..7]                               a (x) b
 *     QNORMALIZE, QSTANDARDIZE q = in[0..3]                                             quaternion
 *     QROT                     q = in[0..3], v = in[4..6]                               vector
 *     QUAT_TO_ROT              q = in[0..3] (any norm > 0)                              3 x 3
 *     QUAT_TO_ROTVEC           q = in[0..3], eps = in[4]                                vector
 *     QUAT_THETA, CALC_HEADING q = in[0..3]                                             angle
 *     QUAT_EXP, EXP_MAP_TO_QUAT  v = in[0..2]                                           quaternion
 *     QUAT_DIFF_MUL            q = in[0..3], omega = in[4..6]                           quaternion
 *     QSLERP                   a = in[0..3], b = in[4..7], t = in[8], one_minus_eps = in[9]   quaternion
 *     CROSS                    a = in[0..2], b = in[3..5]                               a x b
 *     CROSS_ADD                c = in[0..2], a = in[3..5], b = in[6..8]                 c + a x b
 *     M3_V3, TMUL              A = in[0..8], v = in[9..11]                              A v, A^T v
 *     M3_M3                    A = in[0..8], B = in[9..17]                              A B
 * It pins the helpers' source as dm_host.o compiles it; the copies inlined into the step kernels are built under other flags (dm_math_probe.h).
 * Needs no dm_ctx; asynchronous on hip_stream of device device_id.  Refused, nothing is launched: n < 1, a NULL pointer, an op outside [0, DM_MOP_COUNT),
 * no HIP device or a device_id it does not have. */
#define DM_MATH_PROBE_IN 18
#define DM_MATH_PROBE_OUT 12
enum { DM_MOP_SINCOS = 0, DM_MOP_ROT_Y, DM_MOP_ROT_Z, DM_MOP_NORMALIZE_ANGLE, DM_MOP_QMUL, DM_MOP_QNORMALIZE, DM_MOP_QSTANDARDIZE, DM_MOP_QROT, DM_MOP_QUAT_TO_ROT,
       DM_MOP_QUAT_TO_ROTVEC, DM_MOP_QUAT_THETA, DM_MOP_QUAT_EXP, DM_MOP_EXP_MAP_TO_QUAT, DM_MOP_QUAT_DIFF_MUL, DM_MOP_QSLERP, DM_MOP_CALC_HEADING, DM_MOP_CROSS,
       DM_MOP_CROSS_ADD, DM_MOP_M3_V3, DM_MOP_TMUL, DM_MOP_M3_M3, DM_MOP_COUNT };
int dm_math_probe(int device_id, int op, int f64, int n, const double* in_dev, double* out_dev, void* hip_stream);

/* ---- a probe for the wave-level primitives of the step kernels (the top of deepmimic_amd/csrc/dm_device.h and dm_device_duo.h; dm_wave_probe.h): TEST SUPPORT, nothing
 * of the product calls it.  One launch of n_waves workgroups, one wavefront each, evaluates the primitive `op`; lane l of workgroup w reads
 * in_dev[(w * 64 + l) * DM_WAVE_PROBE_IN ..] and writes out_dev[(w * 64 + l) * DM_WAVE_PROBE_OUT ..], doubles both, DEVICE pointers.  Values are narrowed to float
 * (f64 == 0) or kept double on load and widened on store; columns and lanes an op does not write keep the caller's bytes.  "in0" / "in1" are the rows of lanes 0 / 1 of
 * the workgroup (wave-uniform arguments).  `arg` selects among an op's compile-time variants and must be 0 where none is listed.
 *     op            arg                reads                                                        writes (column c)
 *     WAVE_SHFL                        v = in[0], src = in[1] (any int)                             [0] wave_shfl(v, src)
 *     LANE_BCAST                       v = in[0], src_c = in0[1 + c] in 0..63                       c < 63: lane_bcast(v, src_c)
 *     HALF_BCAST                       v = in[0], src_c = in0[1 + c] in 0..31                       c < 63: half_bcast(v, src_c, lane / 32)
 *     HALF_BCAST_C                     v = in[0]                                                    c < 32: half_bcast_c<c>(v, lane / 32)
 *     SHFL_XOR_C                       v = in[0]                                                    c < 6: wave_shfl_xor_c<1 << c>(v)
 *     LANE_SEL      mask chunk         a = in[0], b = in[1]                                         c < 64: lane_sel<mask(arg, c)>(a, b, lane, z)   (wp_mask of dm_wave_probe.h)
 *     ROW_SEL_C                        old = in[0], new = in[1]                                     c < 64: row_sel_c<c>(old, new, lane, one)
 *     HALF_SEL_C                       old = in[0], new = in[1]                                     c < 32: half_sel_c<c>(old, new, lane % 32, one)
 *     CHAIN_KEEP                       v = in[0], lo = in[1], hi = in[2] (uint32 values)            c < 64: chain_keep<c>(v, lo, hi)
 *     ROW_FILE      N: 32 40 48 56 64  x = in[0..N-1], s_k = in0[64 + k], g_k = in1[64 + k]         k < N, 0 <= g_k < N: entry g_k of the file after entry j := x[j] for all j,
 *                                                                                                   then entry s_k := x[k] for k = 0..N-1 in turn where 0 <= s_k < N
 *     BALLOT                           p = in[0] != 0                                               [0], [1] low, high word of wave_ballot(p)
 *     WAVE_SUM, HALF_SUM               v = in[0]                                                    [0] the sum
 *     RCP, RSQRT                       x_c = in[c]                                                  c < 64: dm_rcp(x_c) / dm_rsqrt(x_c)
 *     MED3                             lo, x, hi = in[3c .. 3c + 2]                                 c < 32: dm_med3(lo, x, hi)
 *     WG_UNIT                                                                                       [0] dm_wg_unit() (the grid is n_waves)
 *     GRAM32        NP2: 17 20 32      y = in[0 .. 2 NP2 - 1]                                       c < 32: wave_gram32<NP2>
 *     GRAM64        NP2: 17 32         y                                                            c < 64: wave_gram64_half<NP2, c / 32> entry c % 32
 *     DUO_GRAM32    NP2: 17 20         y                                                            c < 32: duo_gram32<NP2>
 *     XD_OPERANDS                      y (NP2 = 17)                                                 c < 34: y after xd_gram_operands<17>
 *     XD_BLOCK      2 X + Y            y (NP2 = 17)                                                 c < 32: the f(c, value) of xd_gram_block<17, X, Y> after xd_gram_operands
 *     XD_TR_STAGE   stage 0..3         w = in[0..16]                                                c < 17: w after xd_tr_stage<N, MASK, 17>, (N, MASK) = (17, 2) (9, 4) (5, 8) (3, 16)
 * Needs no dm_ctx; asynchronous on hip_stream of device device_id.  Refused, nothing is launched: n_waves < 1 or > 65536, a NULL pointer, an op outside
 * [0, DM_WOP_COUNT), an arg the op does not list, no HIP device or a device_id it does not have. */
#define DM_WAVE_PROBE_IN 128
#define DM_WAVE_PROBE_OUT 64
#define DM_WAVE_PROBE_MASK_CHUNKS 9
enum { DM_WOP_WAVE_SHFL = 0, DM_WOP_LANE_BCAST, DM_WOP_HALF_BCAST, DM_WOP_HALF_BCAST_C, DM_WOP_SHFL_XOR_C, DM_WOP_LANE_SEL, DM_WOP_ROW_SEL_C, DM_WOP_HALF_SEL_C,
       DM_WOP_CHAIN_KEEP, DM_WOP_ROW_FILE, DM_WOP_BALLOT, DM_WOP_WAVE_SUM, DM_WOP_HALF_SUM, DM_WOP_RCP, DM_WOP_RSQRT, DM_WOP_MED3, DM_WOP_WG_UNIT, DM_WOP_GRAM32,
       DM_WOP_GRAM64, DM_WOP_DUO_GRAM32, DM_WOP_XD_OPERANDS, DM_WOP_XD_BLOCK, DM_WOP_XD_TR_STAGE, DM_WOP_COUNT };
int dm_wave_probe(int device_id, int op, int arg, int f64, int n_waves, const double* in_dev, double* out_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
