/*
 * kmanip.h -- C ABI of the MI355X-native batched gym-kmanip hot path.
 *
 * The reference (kscalelabs/gym-kmanip) has no FFI: its backend seam is the Python object
 * returned by `env_sim.new(gym_env)` (reference gym_kmanip/env_base.py:192-200), on which
 * KManipEnv only ever calls k_reset() (env_base.py:221), k_step(action) (env_base.py:242),
 * k_render(cam) (env_base.py:217) and k_close() (env_base.py:266).  This header is what a
 * third backend (`env_hip.new`) binds with ctypes; every entry point cites the reference
 * interface it replaces.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; device buffers are passed as void* device
 *     pointers, the stream as void* (hipStream_t) -- NULL = the null stream.
 *   - every function returns 0 on success, nonzero on error; kmanip_last_error() gives text.
 *   - numerical blow-up of one env is DATA (bit 1 of its done byte), not an error.
 *   - one handle <-> one device; calls on a handle are serialised by the caller
 *     (the reference is single-threaded and non-re-entrant: ik_mujoco.py:34,67).
 *
 * Arithmetic type: float64 on device, like the reference (MuJoCo mjtNum = double,
 * gym_kmanip/__init__.py:50 OBS_DTYPE = float64).  Actions are float32 (__init__.py:51).
 */
#ifndef KMANIP_H
#define KMANIP_H

#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entry points declared in this header (and the diagnostics of
 * kmanip_debug.h) are the ONLY symbols it exports (tests/test_abi.py compares the dynamic symbol table with the two headers). */
#if defined(__GNUC__)
#define KMANIP_API __attribute__((visibility("default")))
#else
#define KMANIP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define KM_MAX_LINKS   20   /* 1-DoF robot links == robot dofs == nu == q_len (10 solo, 20 dual/torso) */
#define KM_MAX_ARMS    2    /* arm 0 = right ("eer"), arm 1 = left ("eel")                         */
#define KM_MAX_IK      7    /* IK unknowns per arm (7 solo/dual, 6 torso)                          */
#define KM_MAX_SPHERES 12   /* sphere colliders per model: per arm two fingers, the palm and three joint housings */
/* Contact slots the solver keeps per step: 4 cube corners on the table, KM_SPHERE_SLOTS sphere-cube contacts and
 * KM_SPHERE_TABLE_SLOTS sphere-table contacts -- the first penetrating spheres in sphere-index order (fingers come first); a
 * further penetrating sphere is dropped for that sub-step (its mask bit stays clear), like the 5th+ cube corner.  Two per arm
 * and kind, except three per arm on the table for the two-arm models, whose hands rest on it.  tests/tools/regime_states.py
 * builds the states that fill them: cell P2 all four sphere-cube slots of a two-arm model, cell T1 both table slots of the single
 * arm and up to four of the six of a two-arm model (tests/test_regimes_gpu.py steps them against the oracle). */
#define KM_SPHERE_SLOTS(nlink) (2 * ((nlink) / 10))
#define KM_SPHERE_TABLE_SLOTS(nlink) ((nlink) >= 20 ? 6 : 2)
#define KM_MAX_CAMS    4    /* cameras: 0 = grip_r, 1 = grip_l, 2 = top, 3 = head (__init__.py:157-161) */
enum { KM_CAM_GRIP_R = 0, KM_CAM_GRIP_L = 1, KM_CAM_TOP = 2, KM_CAM_HEAD = 3 };
#define KM_NQ_CUBE     7
#define KM_NV_CUBE     6

/* action-key columns in the flat [num_envs, act_dim] float32 action matrix; key order is the
 * insertion order of the action Dict space, reference env_base.py:151-188 */
enum {
  KM_ACT_EEL_POS = 0, KM_ACT_EEL_ORN, KM_ACT_EER_POS, KM_ACT_EER_ORN,
  KM_ACT_GRIP_L, KM_ACT_GRIP_R, KM_ACT_QPOS_R, KM_ACT_QPOS_L, KM_ACT_NKEYS
};

enum { KM_JNT_HINGE = 0, KM_JNT_SLIDE = 1 };
enum { KM_SOLVER_PGS = 0, KM_SOLVER_NEWTON = 1 };

/* done byte */
#define KM_DONE_TRUNCATED 1u  /* step_idx reached max_episode_steps (TimeLimit, __init__.py:28,247) */
#define KM_DONE_DIVERGED  2u  /* NaN / |qacc| > 1e10 (dm_control raises PhysicsError instead)       */

/* contact-mask bits (uint32 per env), bit-exact parity target */
#define KM_CON_CUBE_TABLE(c)   (1u << (c))          /* c = 0..7 cube corner vs table plane (<=4 kept) */
#define KM_CON_SPHERE_CUBE(s)  (1u << (8 + (s)))    /* s = sphere index 0..11 (fingers first, then link spheres): sphere vs cube */
#define KM_CON_SPHERE_TABLE(s) (1u << (20 + (s)))   /* sphere vs table plane                                         */
#define KM_CON_ANY_CUBE_TABLE   0x000000FFu
#define KM_CON_ANY_SPHERE_CUBE  0x000FFF00u
#define KM_CON_ANY_SPHERE_TABLE 0xFFF00000u
/* the finger spheres come first in the sphere list, two per arm: "cube touches a gripper finger" (env_sim.py:164-175) */
#define KM_CON_FINGERS_CUBE(nlink) (((1u << (2 * ((nlink) / 10))) - 1u) << 8)

typedef struct KModelDesc {
  /* ---- sizes */
  int32_t nlink;                 /* robot 1-DoF links; nq = nlink + 7, nv = nlink + 6, nu = nlink */
  int32_t narm;                  /* arms present in act_list (0..2)                                */
  int32_t nsphere;
  int32_t act_dim;               /* columns of the action matrix                                   */
  int32_t obs_dim;               /* 2*nlink + 7                                                    */
  int32_t max_episode_steps;     /* 64, __init__.py:28                                             */
  int32_t n_sub_steps;           /* control_timestep / timestep = 10, __init__.py:30, env_sim.py:210 */
  /* Cap on the solver's iterations per solve, MuJoCo's opt.iterations (default 100): PGS sweeps, or Newton iterations of each
   * problem a solve runs (the whole problem of a coupled env; the arm problem, then the cube problem of an uncoupled one, each with
   * a count of its own).  0 = no iteration: qacc is the start point, the cheaper of qacc_warmstart and qacc_smooth (Newton) or
   * qacc_smooth + M^-1 J^T f of the kept warm-start forces (PGS), as in MuJoCo.  (The Newton kernels test the cap after an iteration;
   * for a Newton model with a cap of 0 kmanip_create therefore puts an infinite solver_tolerance into the device's copy of the model,
   * at which the solver's entry test accepts every start point.)  Negative: kmanip_create refuses the descriptor. */
  int32_t solver_iterations;
  int32_t touch_reward_enabled;  /* 0 reproduces the reference's dead touch/lift terms (SURVEY finding 4) */
  int32_t auto_reset;            /* 1: envs whose done byte is set are reset inside kmanip_step    */
  int32_t act_col[KM_ACT_NKEYS]; /* first column of each action key, -1 if the key is absent       */
  int32_t solver;                /* KM_SOLVER_NEWTON (MuJoCo's default, what the reference runs) or KM_SOLVER_PGS */
  /* OPT-IN, NOT THE REFERENCE: cap on the function evaluations of one ik() call.  0 (default) = the reference's
   * scipy.optimize.least_squares default max_nfev = 100 * n (ik_mujoco.py:129-135 passes none): a start in a flat region lets the
   * TRF crawl for 350-650 evaluations, and a batch's launch waits for it (one launch in ~40 at 4096 envs runs 2-7 x long).  A
   * throughput caller may bound it (e.g. 64): the IK then returns its best accepted point with status 0, like SciPy at max_nfev;
   * every parity test and the bench's headline run with 0. */
  int32_t ik_max_nfev;
  int32_t pad0_;

  /* ---- kinematic tree (link i <-> dof i <-> qpos i <-> actuator i), parents before children */
  int32_t link_parent[KM_MAX_LINKS];       /* -1 = fixed to world                                  */
  int32_t jnt_type[KM_MAX_LINKS];
  int32_t forcelimited[KM_MAX_LINKS];
  int32_t pad1_[KM_MAX_LINKS];
  double  link_pos[KM_MAX_LINKS][3];       /* pose in parent link frame (world if parent == -1)    */
  double  link_quat[KM_MAX_LINKS][4];      /* wxyz                                                 */
  double  jnt_axis[KM_MAX_LINKS][3];       /* local                                                */
  double  jnt_range[KM_MAX_LINKS][2];
  double  frictionloss[KM_MAX_LINKS];
  double  kp[KM_MAX_LINKS];
  double  ctrlrange[KM_MAX_LINKS][2];
  double  forcerange[KM_MAX_LINKS][2];
  double  mass[KM_MAX_LINKS];              /* surrogate inertials (build-owned)                    */
  double  com[KM_MAX_LINKS][3];            /* link frame                                           */
  double  inertia[KM_MAX_LINKS][3];        /* diagonal, link-frame axes, about com                 */
  double  q_home[KM_MAX_LINKS];            /* float32-rounded, __init__.py:53-122                  */

  /* ---- arms: arm 0 = right, arm 1 = left */
  int32_t arm_present[KM_MAX_ARMS];
  int32_t arm_nq[KM_MAX_ARMS];
  int32_t arm_q_id[KM_MAX_ARMS][KM_MAX_IK + 1]; /* q_id_r_mask / q_id_l_mask, __init__.py:125-136  */
  int32_t arm_grip_id[KM_MAX_ARMS][2];          /* ctrl_id_*_grip                                  */
  int32_t arm_site_link[KM_MAX_ARMS];
  int32_t arm_mode[KM_MAX_ARMS];                /* 0 = none, 1 = EE-delta + IK, 2 = joint-delta    */
  int32_t arm_has_grip[KM_MAX_ARMS];
  int32_t pad2_[2];
  double  arm_site_pos[KM_MAX_ARMS][3];         /* site pose in its link frame                     */
  double  arm_site_quat[KM_MAX_ARMS][4];

  /* ---- colliders (surrogates): finger + link spheres, table top (height + rectangle), cube box */
  int32_t sphere_link[KM_MAX_SPHERES];
  int32_t sphere_visible[KM_MAX_SPHERES];       /* 1: drawn by the camera renders (fingers); 0: collision only    */
  double  sphere_pos[KM_MAX_SPHERES][3];
  double  sphere_radius[KM_MAX_SPHERES];
  /* Capsule sections: a non-zero sphere_seg[s] makes candidate s, AGAINST THE CUBE, the closest point of the link-fixed segment
   * [sphere_pos, sphere_pos + sphere_seg] to the cube centre (a sphere of the same radius sliding along the link): the forearm /
   * elbow housings are the ends of capsules between consecutive joint origins.  Against the table plane a capsule touches in
   * its end spheres, which are candidates of their own, so that test stays on sphere_pos. */
  double  sphere_seg[KM_MAX_SPHERES][3];
  double  table_z;
  /* The table top is the rectangle x_lo..x_hi, y_lo..y_hi at height table_z (world frame): 0.8 m x 0.4 m centred on the table body
   * -- the plane primitive the reference itself puts in the mesh's place (examples/4_teleop.py:82-84: "table is easier to construct
   * from base vuer plane primitive than load from stl", TABLE_SIZE 0.4 x 0.8 at body "table"; the long side lies along x: the cube
   * spawns at x up to 0.3, __init__.py:164-170).  A cube corner or a sphere touches the table only while its centre line meets the
   * rectangle; beside it, it falls.  +-INFINITY = the round-2 infinite plane. */
  double  table_rect[4];

  /* ---- cube (free body), scene.xml:17-21 */
  double  cube_mass;
  double  cube_inertia[3];
  double  cube_half[3];
  double  cube_frictionloss;
  double  cube_quat0[4];
  double  cube_spawn_lo[3];                     /* __init__.py:164-170                             */
  double  cube_spawn_hi[3];

  /* ---- contact parameters after MuJoCo's pair mixing */
  double  con_cube_solref[2];                   /* pairs involving the cube (condim 4)             */
  double  con_cube_solimp[5];
  double  con_cube_friction[3];                 /* tangential, torsional, rolling                  */
  double  con_def_solref[2];                    /* finger-table pairs (condim 3), joint limits, friction loss */
  double  con_def_solimp[5];
  double  con_def_friction[3];

  /* ---- options / constants */
  double  timestep;                             /* 0.002 (MuJoCo default, no <option> in any XML)  */
  double  gravity[3];
  double  solver_tolerance;                     /* 1e-8                                            */
  double  ik_res_rad, ik_res_reg_prev, ik_res_reg_home, ik_jac_rad, ik_jac_reg; /* __init__.py:37-41 */
  double  ee_pos_delta[3], ee_orn_delta[3];     /* __init__.py:174-187                             */
  double  q_pos_delta;                          /* __init__.py:196                                 */
  double  ee_s_min, ee_s_max, ee_s_delta;       /* __init__.py:199-201                             */
  double  max_q_vel;                            /* pi, __init__.py:31                              */
  double  epsilon;                              /* 1e-6, __init__.py:192                           */
  double  reward_vel_penalty, reward_grip_dist, reward_touch_cube, reward_lift_cube; /* :205-208  */

  /* ---- cameras, all mode="targetbody": gripper cameras on the hand links tracking the EE site body
   * (arm_r_body.xml:68 / arm_l_body.xml:68 / torso_body.xml:104,173) and the world-fixed `top` / `head` cameras
   * tracking the table (_env_solo_arm.xml:11-12 and siblings).  Index = KM_CAM_*.  A link of -1 = world frame.
   * The rendered scene is the build's surrogate geometry = its collision primitives. */
  int32_t cam_present[KM_MAX_CAMS];
  int32_t cam_link[KM_MAX_CAMS];
  int32_t cam_target_link[KM_MAX_CAMS];
  double  cam_pos[KM_MAX_CAMS][3];          /* in cam_link's frame                                    */
  double  cam_target_pos[KM_MAX_CAMS][3];   /* target body origin in cam_target_link's frame          */
  double  cam_fovy[KM_MAX_CAMS];            /* degrees                                                */
  double  cam_znear, cam_zfar;              /* metres; depth is clipped to [znear, zfar], no hit = zfar */

  /* ---- quantities MuJoCo precomputes at qpos0 (mj_setConst): they set the regulariser of every constraint row
   * (efc_diagApprox -> R = (1-d)/d * diagApprox) and the solvers' termination scale 1/(meaninertia * nv).
   * dof_invweight0[i] = (M^-1)_ii; body_invweight0[b] = mean translational / rotational diagonal of J_b M^-1 J_b^T
   * with J_b the 6 x nv Jacobian at body b's centre of mass; the cube (free body): (1/m, mean 1/I_k). */
  double  dof_invweight0[KM_MAX_LINKS];
  double  body_invweight0[KM_MAX_LINKS][2];
  double  cube_invweight0[2];
  double  meaninertia;                      /* trace(M(qpos0)) / nv, all nv = nlink + 6 dofs          */
} KModelDesc;

typedef struct KHandle_* KHandle;

/* sizeof(KModelDesc) as compiled into the library (host bindings check their mirror). */
KMANIP_API int kmanip_model_desc_size(void);

/* Replaces env_sim.new(gym_env) (reference env_sim.py:206-211): build `num_envs` simulated envs
 * on HIP device `device`.  `env_id_offset` is the global index of local env 0 (multi-GPU
 * sharding: RNG streams are keyed by the GLOBAL env id so results do not depend on the shard
 * layout).  The library owns model, state and scratch. */
KMANIP_API int kmanip_create(const KModelDesc* desc, int num_envs, int device, uint64_t seed,
                  int64_t env_id_offset, KHandle* out);
/* Launch shape (no effect on results: an env's bits depend neither on its wave-mates nor on the order its wave is dispatched in --
 * tests compare shards, launch shapes and orders bit for bit).  A step is ONE launch of single-wave workgroups holding 4 (10-link
 * models) or 2 (20-link models) envs each.  When a two-arm handle has more waves than the GPU has SIMD slots (more than 2048 envs),
 * kmanip_step first orders the envs by the cost their last step predicts and dispatches the longest waves first (k_sort_envs, one
 * small extra launch).  A single-arm Newton handle of 2048 or more envs (a multiple of 64) chooses every wave's
 * envs so that no wave holds two predicted to be heavy (SPREAD).  Diagnostic environment variables, each read once
 * by kmanip_create: KMANIP_SPREAD=0 (the identity map instead of SPREAD), KMANIP_COST_SORT=0/1 (force
 * the cost order off / on), KMANIP_EPB=1/2/4 (envs per wave), KMANIP_NO_BLOCK_SPLIT=1 (two-arm inertia as one block),
 * KMANIP_WAVE_CLOCKS=1 (per-wave cycle counts for tests/tools/wave_times.py).
 * Throughput note: one batch's launch ends with its slowest wave and leaves about half the SIMD time idle; handles are
 * independent and every entry point takes the caller's stream, so two or more batches kept in flight on different streams fill
 * it (gym_kmanip_amd/pipeline.py). */

/* Replaces KManipEnvSim.k_reset (env_sim.py:190-194) -> KManipTask.initialize_episode
 * (env_sim.py:23-36): reset envs whose mask byte is nonzero (NULL = all) to the home pose,
 * zero velocity and a fresh cube spawn; writes their observation rows.  mask/obs are device
 * pointers: mask uint8[num_envs], obs double[num_envs, obs_dim] (may be NULL). */
KMANIP_API int kmanip_reset(KHandle h, const uint8_t* mask_dev, double* obs_dev, void* stream);

/* Replaces KManipEnvSim.k_step (env_sim.py:196-200): one control step for every env =
 * KManipTask.before_step (env_sim.py:38-108, incl. ik_mujoco.ik) + physics.step(10)
 * + get_reward (env_sim.py:148-179) + get_observation (env_sim.py:110-146).
 * act_dev float[num_envs, act_dim]; obs_dev double[num_envs, obs_dim];
 * reward_dev double[num_envs]; done_dev uint8[num_envs] (KM_DONE_* bits).  All device memory,
 * owned by the caller. */
KMANIP_API int kmanip_step(KHandle h, const float* act_dev, double* obs_dev, double* reward_dev,
                uint8_t* done_dev, void* stream);

/* State access for parity tests / checkpointing (state is
 * (qpos, qvel, ctrl, qacc_warmstart, time)); HOST pointers, env-major
 * [num_envs, nq|nv|nu|nv], step_idx int32[num_envs]; any pointer may be NULL. Synchronous. */
KMANIP_API int kmanip_get_state(KHandle h, double* qpos, double* qvel, double* ctrl, double* qacc_warm,
                     int32_t* step_idx);
KMANIP_API int kmanip_set_state(KHandle h, const double* qpos, const double* qvel, const double* ctrl,
                     const double* qacc_warm, const int32_t* step_idx);

/* The episode counter completes the checkpoint: the cube-spawn stream is keyed (seed, global env id, episode), so a
 * restored run draws the same spawns as the original only if `episode` is restored too.  HOST int32[num_envs]. Synchronous. */
KMANIP_API int kmanip_get_episode(KHandle h, int32_t* episode);
KMANIP_API int kmanip_set_episode(KHandle h, const int32_t* episode);

/* The state as DEVICE tensors, for any subset of the envs, without leaving the device: what branching
 * rollouts (a planner copies each real env into K candidates), resets to stored states and a policy that reads qvel or ctrl need.
 * All pointers are DEVICE pointers, env-major like kmanip_get_state; any may be NULL (that field is skipped). */
typedef struct KStateDev {
  double*  qpos;       /* [n, nq] */
  double*  qvel;       /* [n, nv] */
  double*  ctrl;       /* [n, nu] */
  double*  qacc_warm;  /* [n, nv] */
  int32_t* step_idx;   /* [n] */
  int32_t* episode;    /* [n] */
} KStateDev;
/* Row j of every tensor is env env_index_dev[j] (DEVICE int32[n]); a NULL index means envs 0 .. n-1.  n >= 0, and n <= num_envs with
 * a NULL index: anything else, or a NULL KStateDev, returns nonzero with kmanip_last_error set and launches nothing; n == 0 succeeds
 * and does nothing.
 * ORDERING: asynchronous on `stream` -- ONE kernel launch for all fields, no host synchronisation, no allocation, no host copy.
 * Enqueued after a kmanip_step on the same stream the call sees that step's result, and a step enqueued after it sees what it
 * wrote; ordering against other streams is the caller's, as everywhere in this header.
 * WHAT IS WRITTEN: kmanip_get_state_dev writes the named rows of the non-NULL tensors.  kmanip_set_state_dev writes the non-NULL
 * fields of the named envs and, if a sim-time buffer is bound (kmanip_bind_sim_time) and step_idx is given, step_idx x
 * control_timestep of those envs; envs the index does not name are not touched, not a bit.  It does NOT touch observations,
 * rewards, done bytes, contact masks or IK diagnostics: a caller that wants those of the new state calls kmanip_observe, as after
 * kmanip_set_state.  The step's scheduling predictors (work counters, SPREAD flags) stay the env's own: they order waves and
 * never change a result.
 * DUPLICATES: an env named twice in a read is fine (that is the broadcast).  An env named twice as a DESTINATION ends with, in
 * every component, the value of ONE of the rows that name it -- which one is unspecified and may differ between components.
 * OUT-OF-RANGE INDICES: an entry outside 0 .. num_envs-1 is never used as an address; its row is skipped (not read, not
 * written) and a counter the handle owns is incremented (kmanip_state_index_errors); every other entry is carried out.  The call
 * still returns 0: the index lives on the device.
 * ERRORS: a refused call leaves the handle exactly as it was. */
KMANIP_API int kmanip_get_state_dev(KHandle h, const int32_t* env_index_dev, int n, const KStateDev* out, void* stream);
KMANIP_API int kmanip_set_state_dev(KHandle h, const int32_t* env_index_dev, int n, const KStateDev* in, void* stream);

/* Env to env on the device: env dst_index_dev[j] of `dst` receives qpos, qvel, ctrl, qacc_warm and step_idx of env
 * src_index_dev[j] of `src` (DEVICE int32[n] each; NULL = 0 .. n-1, then n <= that handle's num_envs), and the bound sim time of
 * `dst` is updated as by kmanip_set_state_dev.  Rows, ordering (on `stream`, for BOTH handles), untouched envs, duplicates and the
 * things not copied (observations, rewards, done bytes, contact masks, IK diagnostics, scheduling predictors) are as above; a bad
 * entry on either side skips that entry and counts on the DESTINATION handle.  ONE launch.
 *   KM_COPY_EPISODE     the episode counter travels too (without it the destination's counters stay).
 *   KM_COPY_ENV_PARAMS  the KM_EP_* values in force for the source env travel too (in ranges mode: those drawn for its current
 *                       episode).  `src` has per-env parameters and `dst` has none: nonzero, "destination has no per-env
 *                       parameters: call kmanip_set_env_params first", nothing launched.  `src` has none and `dst` has them: the
 *                       destination envs get the compiled model's values.  Neither has them: the flag does nothing.  A
 *                       destination in ranges mode keeps the copied values until its next reset redraws them (the rule of
 *                       kmanip_set_env_param_ranges).
 * RANDOM STREAMS STAY PER ENV: the spawn, action and parameter streams are keyed by the DESTINATION handle's seed and the
 * destination env's own global env id (env_id_offset + index), neither of which is copied, so a clone stepped with its source's actions follows it bit for bit only until either of them is reset
 * (the TimeLimit's auto-reset included): from there the two draw different cubes.
 * COMPATIBILITY: the two handles must be on one device and their KModelDesc byte-equal; otherwise nonzero with kmanip_last_error
 * set on `dst`, nothing launched.
 * SAME HANDLE: dst == src is allowed for any index pair, permutations included, and gives what reading every source row first and
 * writing afterwards gives: the rows pass through a staging copy the handle owns (two launches of the same kernel).  The staging
 * copy is allocated by the FIRST same-handle call (and again only by one with n larger than num_envs and than every n before):
 * that call alone waits for the whole device; every other one is asynchronous like the rest.  A handle has ONE staging copy:
 * two same-handle calls on different streams must be ordered by the caller like any two writers of one buffer. */
enum { KM_COPY_EPISODE = 1, KM_COPY_ENV_PARAMS = 2 };
KMANIP_API int kmanip_copy_envs(KHandle dst, const int32_t* dst_index_dev, KHandle src, const int32_t* src_index_dev,
                     int n, unsigned flags, void* stream);
/* The number of index entries the three calls above skipped on this handle since the last call of this function, which also
 * clears it.  The counter lives on the device (allocated by kmanip_create).  Synchronous: waits for the whole device. */
KMANIP_API int kmanip_state_index_errors(KHandle h, int64_t* count);

/* Asynchronous device-to-device copy of the per-env counters into caller-owned DEVICE buffers (int32[num_envs] each, either
 * may be NULL) on `stream`: lets the k_step seam return sim_time (= step_idx * control_timestep, env_sim.py:194,200) as a
 * device tensor without synchronising. */
KMANIP_API int kmanip_get_counters(KHandle h, int32_t* step_idx_dev, int32_t* episode_dev, void* stream);

/* Bind a caller-owned DEVICE buffer double[num_envs] that every kmanip_step / kmanip_reset also fills with the env's
 * simulation time (dm_control's data.time, the last element of k_step's return tuple, env_sim.py:194,200) =
 * steps since the env's last reset x control_timestep.  NULL unbinds.  The buffer must outlive the binding. */
KMANIP_API int kmanip_bind_sim_time(KHandle h, double* sim_time_dev);

/* MuJoCo's data.qfrc_applied.  qfrc_dev: DEVICE double[num_envs, nv], env-major, nv = nlink + 6, caller-owned;
 * NULL unbinds.
 * ROW LAYOUT (the dof order of qM / qfrc_bias in kmanip_kinematics): columns 0 .. nlink-1 joint torque (hinge) or force (slide);
 * nlink .. nlink+2 force on the cube at its centre of mass, world frame; nlink+3 .. nlink+5 torque on the cube in the cube's BODY
 * frame (free-joint convention).
 * THE STEP: while a buffer is bound, every sub-step of kmanip_step and kmanip_step_chunk adds row `env` to the smooth right-hand side
 * (rhs = -bias + servo force + applied), with both solvers, the first sub-step (which uses the pre-IK products) included.  The force is
 * not clamped by forcerange or ctrlrange: those limit actuators.  The buffer is read once per launch, at the env's load; a chunk holds
 * it for all its steps.  Ordering is the stream's: a write enqueued before the step on the step's stream is seen.  The bind itself is a
 * host-side switch, like kmanip_bind_sim_time; the buffer must outlive the binding.  A buffer of zeros gives the bits of no buffer.
 * WHAT THE LIBRARY DOES NOT DO WITH IT: it never writes the buffer and never clears it.  It is not state: kmanip_get/set_state*,
 * kmanip_copy_envs, checkpoints and snapshots do not carry it.  Resets ignore it: kmanip_reset and the auto-reset's forward pass
 * (actuation disabled) compute what they compute without a buffer, bit for bit (MuJoCo's mj_resetData zeroes qfrc_applied; here the
 * caller zeroes the rows of done envs if it wants that).
 * kmanip_forces honours the buffer; kmanip_kinematics and kmanip_observe do not depend on it.
 * NON-FINITE COMPONENTS are data, not an error: the check runs at the env's load, before any solver.  Such an env is treated as
 * diverged for that step -- KM_DONE_DIVERGED, zero observation and reward, empty contact mask, the usual reset of a diverged env -- and
 * gets status 1 with zero outputs from kmanip_forces; every other env is untouched, bit for bit.
 * ERRORS: a NULL handle returns nonzero.  The pointer cannot be validated on the host.  Scheduling predictors keep working on what
 * they already measure. */
KMANIP_API int kmanip_bind_applied_force(KHandle h, const double* qfrc_dev);

/* The multi-GPU learner's per-step exchange is one packed record per env, (reward, done as a double), all-gathered across the
 * ranks (gym_kmanip_amd/dist.py).  Bound here, every kmanip_step writes that record itself into ONE of two
 * caller-owned double[num_envs, 2] buffers -- the one chosen by kmanip_select_reward_done_record (rec0 after the bind) -- so that
 * the exchange costs the step's stream no packing kernel.  reward_dev / done_dev are written as always.  NULL, NULL unbinds;
 * kmanip_step_chunk does not write records.
 * ORDERING INVARIANT (the caller's): a collective that still READS buffer b must have completed -- or the step's stream must have
 * been made to wait for it -- BEFORE the kmanip_step that fills b is enqueued; two buffers only mean that step k may overlap
 * the exchange of step k-1, not that no wait is needed (dist.RewardDoneGather.before_step).  The library keeps no counter of
 * its own: a step without an exchange (evaluation, a failed launch) cannot put the two sides out of phase. */
KMANIP_API int kmanip_bind_reward_done_record(KHandle h, double* rec0_dev, double* rec1_dev);
/* index 0 / 1: the bound buffer the following kmanip_step calls fill. */
KMANIP_API int kmanip_select_reward_done_record(KHandle h, int index);

/* KManipTask.get_observation + get_reward (env_sim.py:110-179) of every env's CURRENT state, without stepping -- what
 * dm_control evaluates after a physics.forward(): obs_dev double[num_envs, obs_dim], reward_dev double[num_envs] (either may be
 * NULL); the contact masks kmanip_get_diag returns are refreshed too.  An env whose qpos / qvel hold a non-finite value (a restored
 * diverged checkpoint) gets what kmanip_step reports for a diverged env: zero observation, zero reward, an empty contact mask.  Used by the parity tests against fixtures made from the
 * reference's own Python (tests/golden/ref_obs_*.npz) and by callers that restore a checkpoint with kmanip_set_state. */
KMANIP_API int kmanip_observe(KHandle h, double* obs_dev, double* reward_dev, void* stream);

/* Contact forces, qacc and joint forces of every env's CURRENT state: mj_forward with actuation at the env's
 * (qpos, qvel, ctrl) -- what dm_control's physics.forward() followed by data.qacc, data.qfrc_constraint, data.qfrc_actuator and
 * mj_contactForce of every contact gives.  nv = nlink + 6, nu = nlink, NC = KM_CONTACT_SLOTS(nlink).
 * All pointers are DEVICE pointers, env-major; any may be NULL (that field is skipped). */
#define KM_CONTACT_SLOTS(nlink) (4 + KM_SPHERE_SLOTS(nlink) + KM_SPHERE_TABLE_SLOTS(nlink))   /* 8 / 14 */
typedef struct KForcesDev {
  double*   qacc;             /* [n, nv] */
  double*   qfrc_constraint;  /* [n, nv]  = M (qacc - qacc_smooth): the joint-space sum of every constraint force (contacts, limits, friction loss) */
  double*   qfrc_actuator;    /* [n, nu]  clamped servo force, per-env kp scale honoured */
  double*   contact_force;    /* [n, NC, 4] normal, tangent 1, tangent 2, torsion, in the contact frame; condim-3 pair: torsion 0 */
  int32_t*  contact_bit;      /* [n, NC]  the KM_CON_* bit index (0..31) of the pair in this slot, -1 = empty slot (its other fields 0) */
  double*   contact_frame;    /* [n, NC, 9] rows normal, t1, t2 (world) */
  double*   contact_pos;      /* [n, NC, 3] */
  double*   contact_dist;     /* [n, NC] */
  uint32_t* contact_mask;     /* [n] */
  uint8_t*  status;           /* [n] 0 ok; 1 = non-finite state or failed factorisation / bad qacc: every other output of the env is 0
                               *     and every slot empty (contact_bit -1); also a non-finite component in the env's bound applied force */
} KForcesDev;
/* ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  Enqueued after a kmanip_step on the
 * same stream it sees that step's result.
 * SIGN: the frame normal points from the first body of the pair to the second -- table -> cube, link -> cube, table -> link.  The force
 * acts on the second body along +frame and on the first with the opposite sign: the net contact force on the cube in the world frame
 * is the sum of F0 n + F1 t1 + F2 t2 over the slots whose bit is a cube pair (KM_CON_ANY_CUBE_TABLE | KM_CON_ANY_SPHERE_CUBE).
 * A slot's four numbers are the sums of its pyramid-edge forces along its basis rows (mj_contactForce): F0 >= 0, |F1|, |F2| <= mu F0,
 * |F3| <= mu_torsion F0.
 * SLOT ORDER: only the kinds are fixed -- 4 cube-corner slots, then KM_SPHERE_SLOTS sphere-cube, then KM_SPHERE_TABLE_SLOTS
 * sphere-table; contact_bit says who sits where, and callers index by bit.  The occupied slots are exactly the bits of contact_mask.
 * INPUTS: ctrl is used exactly as stored (the float32 rounding that starts kmanip_step's before_step is not applied); the stored
 * qacc_warm is the solver's starting point.  A bound applied force (kmanip_bind_applied_force) is honoured: qacc and qfrc_constraint =
 * M (qacc - qacc_smooth) are those of the forced state, and M qacc + qfrc_bias = qfrc_actuator (padded with six zeros) + qfrc_applied +
 * qfrc_constraint with kmanip_kinematics' qM and qfrc_bias; an env whose row has a non-finite component gets status 1.  After an auto-reset the forces are those of the new episode's first state.  Per-env
 * parameters (KM_EP_*) are honoured, explicit and ranges mode alike.
 * THE HANDLE IS READ ONLY: state, warm start, counters, the contact masks kmanip_get_diag returns, scheduling predictors, sim time and
 * random streams stay bit for bit as they were; a step after the call is the step without it.
 * ERRORS: a NULL handle, a NULL `out` or a handle whose solver is KM_SOLVER_PGS ("contact forces need the Newton solver") return
 * nonzero with kmanip_last_error set and launch nothing.  Every field NULL: the call succeeds and does nothing. */
KMANIP_API int kmanip_forces(KHandle h, const KForcesDev* out, void* stream);

/* Link and site poses, site Jacobians, joint-space inertia and bias forces of every env's CURRENT state: what a
 * dm_control user reads off physics.data after physics.forward() -- data.xpos / data.xmat of the link bodies, site("eer_site_pos").xpos
 * / .xmat (examples/2_synthetic_data.py:34, env_sim.py:63-90), mj_jacSite (ik_mujoco.py:74), mj_fullM and data.qfrc_bias.
 * nlink = KModelDesc::nlink, nv = nlink + 6 (the cube's six dofs last).  All pointers are DEVICE pointers, env-major; any may be NULL
 * (that field is skipped). */
typedef struct KKinDev {
  double*  link_xpos;   /* [n, nlink, 3]  MuJoCo data.xpos of the link bodies                        */
  double*  link_xmat;   /* [n, nlink, 9]  data.xmat, row-major                                       */
  double*  site_xpos;   /* [n, KM_MAX_ARMS, 3]  eer / eel site (arm 0 = right); absent arm: zeros    */
  double*  site_xmat;   /* [n, KM_MAX_ARMS, 9]                                                       */
  double*  site_jacp;   /* [n, KM_MAX_ARMS, 3, nv]  mj_jacSite, world frame, all nv columns          */
  double*  site_jacr;   /* [n, KM_MAX_ARMS, 3, nv]                                                   */
  double*  site_vel;    /* [n, KM_MAX_ARMS, 6]  jacp qvel, then jacr qvel (world frame)              */
  double*  qM;          /* [n, nv, nv]  dense joint-space inertia (mj_fullM), cube block included    */
  double*  qfrc_bias;   /* [n, nv]      Coriolis + centrifugal + gravity, cube rows included         */
  uint8_t* status;      /* [n] 0 ok; 1 = non-finite qpos/qvel: every other output of the env is 0    */
} KKinDev;
/* LAUNCH: ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  Enqueued after a kmanip_step
 * on the same stream it sees that step's result.
 * INPUTS: the stored qpos and qvel as they are.  ctrl and the warm start have no influence on any output.
 * PER-ENV PARAMETERS (KM_EP_*) are honoured, explicit and ranges mode alike: the cube's mass and inertia enter qM's cube block and the
 * cube rows of qfrc_bias (nothing else here depends on a parameter).
 * BOTH SOLVERS: nothing here depends on the solver; a KM_SOLVER_PGS handle is served (unlike kmanip_forces) and returns the bits a
 * Newton handle returns.
 * JACOBIANS: column j is non-zero only for the dofs of links that are ancestor-or-self of arm_site_link[a] -- all of them, not only
 * arm_q_id[a] (the Torso's sites sit on the hand joints 10 / 19, which the IK does not move).  Hinge j: axis_j x (site - xpos_j) in jacp and axis_j in jacr; slide j:
 * axis_j in jacp and 0 in jacr (axis_j the joint's axis in the world frame).  Every other column, the six cube columns included, is
 * exactly 0.0; so is everything of an absent arm.  site_vel = [jacp qvel, jacr qvel].
 * qM: bitwise symmetric, exact zeros between the two arms' trees and between robot and cube; cube block = diag(m, m, m, I0, I1, I2)
 * (the cube's angular velocity is expressed in its body frame, MuJoCo's free-joint convention).  The operational-space inertia is
 * not computed: callers form (J M^-1 J^T)^-1 from these tensors.
 * qfrc_bias: what MuJoCo's mj_rne gives without acceleration; M qacc + qfrc_bias = qfrc_actuator (padded with six zeros) +
 * qfrc_constraint with the tensors of kmanip_forces.
 * THE HANDLE IS READ ONLY: nothing of the handle's state is written (state, warm start, counters, contact masks, scheduling
 * predictors, sim time, random streams); a step after the call is the step without it.
 * ERRORS: a NULL handle or a NULL `out` return nonzero with kmanip_last_error set and launch nothing.  Every field NULL: the call
 * succeeds and does nothing.
 * OUT OF SCOPE: render snapshots, centre-of-mass Jacobians.  (Env subsets and hypothetical states: kmanip_kinematics_rows below.) */
KMANIP_API int kmanip_kinematics(KHandle h, const KKinDev* out, void* stream);

/* Inverse dynamics of a GIVEN acceleration: MuJoCo's mj_inverse / data.qfrc_inverse.  Per env, at the state
 * (qpos, qvel) and for qacc in the dof order of qM / qfrc_bias:
 *     f(qacc)         = the constraint rows' forces at x = J qacc - aref: friction-loss rows saturating at +-floss, limit rows and
 *                       pyramid edges one-sided (-x / R for x < 0, else 0)
 *     qfrc_constraint = J^T f(qacc)
 *     qfrc_inverse    = M qacc + qfrc_bias - qfrc_constraint
 * The soft constraints make f a closed-form function of qacc: nothing is solved.  There is no passive force in this model (friction
 * loss is a constraint row), so qfrc_inverse is the TOTAL generalised force that produces qacc: at the forward solution it equals
 * qfrc_actuator (padded with six zeros) + qfrc_applied of kmanip_forces, and bound as the applied force on top of the servos
 * (minus their qfrc_actuator) it makes kmanip_forces return qacc, the forward problem being strictly convex.
 * nv = nlink + 6, nq = nlink + 7, NC = KM_CONTACT_SLOTS(nlink).  All pointers are DEVICE pointers, env-major, row e = env e. */
typedef struct KInverseIn {
  const double* qacc;   /* [n, nv] row-major, required */
  const double* qpos;   /* [n, nq] or NULL: the handle's state */
  const double* qvel;   /* [n, nv] or NULL */
} KInverseIn;
typedef struct KInverseDev {
  double*   qfrc_inverse;     /* [n, nv] */
  double*   qfrc_constraint;  /* [n, nv] */
  double*   contact_force;    /* [n, NC, 4] normal, t1, t2, torsion: the decode and sign convention of KForcesDev::contact_force */
  int32_t*  contact_bit;      /* [n, NC], -1 = empty */
  uint32_t* contact_mask;     /* [n] */
  uint8_t*  status;           /* [n] 0 ok; 1 = non-finite state or qacc, or a failed factorisation of M: every other output of the env
                               *     is 0 and every slot empty (contact_bit -1) */
} KInverseDev;
/* ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  Any output may be NULL (that field is
 * skipped); every field NULL: the call succeeds and does nothing.
 * INPUTS: a given qpos / qvel replaces the handle's for this call only, used exactly as kmanip_set_state_dev followed by the call would
 * use it (the quaternion as stored: the kinematics normalise it as they do in a step).  ctrl, the warm start and a bound applied
 * force do not enter.  Per-env parameters (KM_EP_*) are honoured, explicit and ranges mode alike.
 * SLOTS: order, contact_bit, contact_mask and the sign of contact_force are those of kmanip_forces, which also keeps the contact
 * geometry (frame, point, distance): it does not depend on qacc.
 * BOTH SOLVERS: nothing is solved, and the rows are always those of the Newton path's assembly (the primal rows of the oracle); a
 * KM_SOLVER_PGS handle is served and returns the bits a Newton handle returns.
 * THE HANDLE IS READ ONLY: state, warm start, counters, contact masks, scheduling predictors, sim time and random streams stay bit for
 * bit as they were; a step after the call is the step without it.
 * ERRORS: a NULL handle, a NULL `in`, a NULL `out` or a NULL in->qacc return nonzero with kmanip_last_error set and launch nothing. */
KMANIP_API int kmanip_inverse(KHandle h, const KInverseIn* in, const KInverseDev* out, void* stream);

/* Forward dynamics at rows the CALLER passes, as many as it likes: MuJoCo's mj_forward on a scratch mjData.
 * What kmanip_forces computes for the state a handle holds, one row per env, this computes for n rows of hypothetical states: row r
 * names an env and gives, per field, its own values or none.  nq = nlink + 7, nv = nlink + 6, nu = nlink.  All pointers are DEVICE
 * pointers, row-major. */
typedef struct KForwardIn {
  const int32_t* env_index;    /* [n] DEVICE: row r takes model parameters (KM_EP_*) and every NULL field below from env env_index[r];
                                  NULL = rows 0 .. n-1 are envs 0 .. n-1, and then n <= num_envs */
  const double*  qpos;         /* [n, nq] or NULL: the named env's stored qpos */
  const double*  qvel;         /* [n, nv] or NULL */
  const double*  ctrl;         /* [n, nu] or NULL; used exactly as given / stored, no float32 rounding (kmanip_forces' rule) */
  const double*  qacc_warm;    /* [n, nv] or NULL: the named env's stored warm start */
  const double*  qfrc_applied; /* [n, nv] or NULL: the named env's row of a bound applied force, none if nothing is bound */
} KForwardIn;
/* OUTPUTS: KForcesDev with n rows in place of num_envs, written at the ROW; every field keeps its meaning, sign convention and slot
 * order (kmanip_forces above); any field may be NULL, every field NULL: the call succeeds and does nothing.
 * status: 0 ok; 1 = a non-finite value in any input the row uses (given or stored), a failed factorisation or a bad qacc, tested as
 * kmanip_forces tests it; 2 = env_index[r] lies outside 0 .. num_envs-1: the entry is never used as an address, and the call still
 * returns 0.  With status 1 or 2 every other output of the row is 0 and every slot empty (contact_bit -1).  The counter of
 * kmanip_state_index_errors keeps its meaning and is not touched.
 * ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  Enqueued after a kmanip_step on the
 * same stream it sees that step's result.
 * n >= 0; n == 0 succeeds and does nothing.  n may exceed num_envs when an index is given, and the same env may be named in any
 * number of rows.  A given row replaces the env's for this call only and is used exactly as kmanip_set_state_dev followed by
 * kmanip_forces would use it (the quaternion as stored: the kinematics normalise it as they do in a step).
 * THE INVARIANT: with every input field NULL and n == num_envs, a row computes what kmanip_forces computes for that env, the bound
 * applied force and per-env parameters (explicit and ranges mode alike) included.
 * THE HANDLE IS READ ONLY: state, warm start, counters, the contact masks kmanip_get_diag returns, scheduling predictors, sim time and
 * random streams stay bit for bit as they were; a step after the call is the step without it.
 * ERRORS: a NULL handle, a NULL `in`, a NULL `out`, n < 0, n > num_envs with a NULL env_index, or a handle whose solver is
 * KM_SOLVER_PGS ("contact forces need the Newton solver": the rows are solved by the Newton path) return nonzero with
 * kmanip_last_error set and launch nothing.
 * OUT OF SCOPE: discrete-time transition matrices, analytic derivatives (gym_kmanip_amd/derivatives.py builds finite differences from
 * two calls).  (Kinematics at rows: kmanip_kinematics_rows below.) */
KMANIP_API int kmanip_forward(KHandle h, const KForwardIn* in, int n, const KForcesDev* out, void* stream);

/* Kinematics at rows the CALLER passes, as many as it likes: what kmanip_kinematics computes for the state a
 * handle holds, one row per env, this computes for n rows of hypothetical states -- the nominal trajectories of an iLQR iteration, the
 * rows of its line search.  Row r names an env and gives its own qpos / qvel or none.  nq = nlink + 7, nv = nlink + 6.  All pointers
 * are DEVICE pointers, row-major. */
typedef struct KKinRowsIn {
  const int32_t* env_index;  /* [n] DEVICE: row r takes per-env parameters (KM_EP_*) and every NULL field below from env env_index[r];
                                NULL = rows 0 .. n-1 are envs 0 .. n-1, and then n <= num_envs */
  const double*  qpos;       /* [n, nq] or NULL: the named env's stored qpos */
  const double*  qvel;       /* [n, nv] or NULL */
} KKinRowsIn;
/* OUTPUTS: KKinDev with n rows in place of num_envs, written at the ROW; every field keeps its meaning (kmanip_kinematics above); any
 * field may be NULL, every field NULL: the call succeeds and does nothing.
 * status: 0 ok; 1 = a non-finite qpos or qvel the row uses, given or stored (kmanip_kinematics' test; ctrl and the warm start do not
 * enter); 2 = env_index[r] lies outside 0 .. num_envs-1: the entry is never used as an address, and the call still returns 0.  With
 * status 1 or 2 every other output of the row is 0.
 * ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  n >= 0; n == 0 succeeds and does
 * nothing.  n may exceed num_envs when an index is given, and the same env may be named in any number of rows.  A given row is used
 * exactly as kmanip_set_state_dev followed by kmanip_kinematics would use it.  Where neither qM nor qfrc_bias is wanted the tree passes
 * behind the forward kinematics are skipped; the other fields' bits do not depend on that.
 * PER-ENV PARAMETERS of the named env are honoured: the cube's mass and inertia enter qM's cube block and the cube rows of qfrc_bias.
 * BOTH SOLVERS: a KM_SOLVER_PGS handle is served and returns the bits a Newton handle returns.
 * THE INVARIANT: with every input field NULL and n == num_envs, a row holds kmanip_kinematics' bits for that env.
 * THE HANDLE IS READ ONLY, as for kmanip_kinematics.
 * ERRORS: a NULL handle, a NULL `in`, a NULL `out`, n < 0, or n > num_envs with a NULL env_index return nonzero with kmanip_last_error
 * set and launch nothing. */
KMANIP_API int kmanip_kinematics_rows(KHandle h, const KKinRowsIn* in, int n, const KKinDev* out, void* stream);

/* A site-pose cost of n rows of hypothetical states, its gradient and its Gauss-Newton Hessian in ONE launch: the
 * task-space cost of an iLQR iteration.  For row r, summed over the present arms a, in the tangent x = [dq (nv) ; qvel (nv)] of
 * kmanip_transition_fd, nx = 2 nv:
 *     p*_a    = target_pos[r, a] + follow_cube[a] * cube_pos(r)
 *     e_pos_a = site_xpos_a - p*_a
 *     e_rot_a = the rotation vector w (|w| <= pi, world frame) with exp([w]x) = R_site_a R_target_a^T
 *     cost    = 1/2 sum_a ( weight[r, a, 0] |e_pos_a|^2 + weight[r, a, 1] |e_rot_a|^2 )
 *     Jp_a    = site_jacp_a on the arm columns, -follow_cube[a] I on the cube's position columns nlink .. nlink+2, 0 elsewhere
 *     Jr_a    = site_jacr_a, 0 on all six cube columns
 *     lx[j]     = sum_a ( w0 e_pos_a . Jp_a[:, j] + w1 e_rot_a . Jr_a[:, j] )                 for j < nv, 0 for j >= nv
 *     lxx[i, j] = sum_a sum_c ( w0 Jp_a[c, i] Jp_a[c, j] + w1 Jr_a[c, i] Jr_a[c, j] )        for i, j < nv, 0 elsewhere
 * R_target is the rotation of target_quat[r, a] (wxyz), normalised; it is read only where weight[r, a, 1] != 0, and a NULL target_quat
 * makes every rotation weight count as 0.  The gradient is exact for both terms (e_rot is an eigenvector, eigenvalue 1, of the log
 * map's Jacobian); the Hessian drops the second-order terms.  Targets and weights are per row: a caller sets terminal weights and
 * time-varying targets by filling rows.  All pointers are DEVICE pointers, row-major. */
typedef struct KSiteCostIn {
  const int32_t* env_index;   /* [n] or NULL: KKinRowsIn's */
  const double*  qpos;        /* [n, nq] or NULL: the named env's stored qpos */
  const double*  target_pos;  /* [n, KM_MAX_ARMS, 3], required */
  const double*  target_quat; /* [n, KM_MAX_ARMS, 4] or NULL */
  const double*  weight;      /* [n, KM_MAX_ARMS, 2] (position, rotation), required */
  int32_t        follow_cube[KM_MAX_ARMS];   /* nonzero: the arm's target position is an offset from the cube's */
} KSiteCostIn;
typedef struct KSiteCostDev { /* any field may be NULL */
  double*  cost;       /* [n] */
  double*  lx;         /* [n, nx] */
  double*  lxx;        /* [n, nx, nx] */
  double*  site_xpos;  /* [n, KM_MAX_ARMS, 3]  absent arm: zeros */
  double*  resid;      /* [n, KM_MAX_ARMS, 6]  e_pos, e_rot; absent arm: zeros */
  uint8_t* status;     /* [n] */
} KSiteCostDev;
/* LAUNCH, rows, the env index, n, per-env parameters, both solvers and the read-only handle: kmanip_kinematics_rows' rules.  qvel
 * does not enter: a stored non-finite velocity does not spoil a cost at a given qpos.  An absent arm's targets and weights are never
 * read.
 * status: 0 ok; 1 = a non-finite qpos the row uses, given or stored, or a non-finite target or weight of a present arm; 2 = an env
 * index out of range.  With status 1 or 2 every other output of the row is 0.
 * lxx: every entry of a wanted row is written, exact +0.0 outside the nv x nv block; each entry is one FMA chain in a fixed order (arm
 * 0 position c = 0 .. 2, arm 0 rotation, then arm 1) of terms w (J[c, i] J[c, j]) with the product rounded first, so the matrix is
 * bitwise symmetric and a row's result does not depend on n, on its index or on its neighbours.
 * ERRORS: kmanip_kinematics_rows', and a NULL target_pos or weight.
 * OUT OF SCOPE: velocity-space site costs, link poses other than the two sites, following the cube's orientation, a cross term lux. */
KMANIP_API int kmanip_site_cost(KHandle h, const KSiteCostIn* in, int n, const KSiteCostDev* out, void* stream);

/* Open-loop rollouts in ctrl space from rows the CALLER passes, as many as it likes: MuJoCo's `rollout` module
 * on scratch mjData.  Row r names an env and gives, per field, its own values or none (KForwardIn's fields and NULL semantics); it is
 * then integrated for nstep steps of nsub sub-steps each, and the state after every step is recorded at the row.  nq = nlink + 7,
 * nv = nlink + 6, nu = nlink.  All pointers are DEVICE pointers, row-major. */
typedef struct KRolloutIn {
  const int32_t* env_index;    /* [n] DEVICE: row r takes model parameters (KM_EP_*) and every NULL field below from env env_index[r];
                                  NULL = rows 0 .. n-1 are envs 0 .. n-1, and then n <= num_envs */
  const double*  qpos;         /* [n, nq] or NULL: the named env's stored qpos */
  const double*  qvel;         /* [n, nv] or NULL */
  const double*  qacc_warm;    /* [n, nv] or NULL: the named env's stored warm start (the first sub-step's; later ones carry their own) */
  const double*  ctrl;         /* ctrl_per_step ? [n, nstep, nu] : [n, nu], or NULL: the named env's stored ctrl, held.  Used exactly
                                  as given (float64): no action decode, no IK, no CTRL_ALPHA filter, no float32 rounding; the servos'
                                  ctrlrange / forcerange clamps act as they do in every sub-step */
  const double*  qfrc_applied; /* frc_per_step ? [n, nstep, nv] : [n, nv], or NULL: the named env's row of a bound applied force, held,
                                  none if nothing is bound */
  int32_t ctrl_per_step;       /* 1: row (r, t) of ctrl acts during step t; 0: row r is held for all steps */
  int32_t frc_per_step;        /* likewise for qfrc_applied */
} KRolloutIn;
/* OUTPUTS, written at the ROW; any field may be NULL. */
typedef struct KRolloutDev {
  double*   qpos;          /* [n, nstep, nq] the state after each step */
  double*   qvel;          /* [n, nstep, nv] */
  double*   qacc_warm;     /* [n, nstep, nv] the warm start the next step would begin from (the last sub-step's qacc) */
  uint32_t* contact_mask;  /* [n, nstep] KM_CON_* bits of the state after the step (the step kernel's trailing mj_step1) */
  double*   reward;        /* [n, nstep] the env's get_reward at the state after the step; the trailing kinematics + collision pass
                              that feeds mask and reward is skipped when both are NULL */
  uint8_t*  status;        /* [n] 0: the row ran all steps; 1: a non-finite input the row uses (given or stored, of any step), a failed
                              factorisation, a bad qacc or a non-finite qpos -- the step kernel's divergence tests and kmanip_forward's
                              input tests; 2: env_index[r] lies outside 0 .. num_envs-1: the entry is compared before it is ever used
                              as an address, and the call still returns 0 */
  int32_t*  steps_done;    /* [n] whole steps recorded before the row stopped (nstep with status 0).  A row that diverges stops there:
                              its records from step steps_done on are zeros, contact_mask 0.  It never resets and draws no random
                              number */
} KRolloutDev;
/* ONE STEP is nsub sub-steps: mj_step1's products, the solve with actuation, the bad-qacc test, mj_Euler -- kmanip_step's sub-step loop
 * with nothing teleported, so every sub-step is a plain mj_step; the warm start carries from sub-step to sub-step.  nsub == 0 means
 * the model's n_sub_steps (one record per control step); nsub == 1 is MuJoCo's own granularity.
 * BOTH SOLVERS: the rollout runs the handle's solver, so that it predicts the handle's own step.
 * ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.
 * n may exceed num_envs when an index is given, and the same env may be named in any number of rows.  n == 0 or nstep == 0 succeeds
 * and does nothing.  The counter of kmanip_state_index_errors keeps its meaning and is not touched.
 * THE HANDLE IS READ ONLY: state, warm start, counters, the contact masks kmanip_get_diag returns, scheduling predictors, sim time and
 * random streams stay bit for bit as they were; a step after the call is the step without it.
 * ERRORS: a NULL handle, a NULL `in`, a NULL `out`, n < 0, nstep < 0, nsub < 0, n > num_envs with a NULL env_index, or a per-step flag
 * set on a NULL tensor return nonzero with kmanip_last_error set and launch nothing.
 * OUT OF SCOPE: action-space rollouts (kmanip_step_chunk on a cloned handle), observations per step, analytic derivatives, rollouts
 * that continue through a reset (gym_kmanip_amd/derivatives.py transition_fd builds A = ds'/ds, B = ds'/du from two calls). */
KMANIP_API int kmanip_rollout(KHandle h, const KRolloutIn* in, int n, int nstep, int nsub, const KRolloutDev* out, void* stream);

/* Closed-loop rollouts: kmanip_rollout with a per-step affine state feedback evaluated on the device -- the
 * time-varying policy of an iLQR / DDP backward pass, a regulator that holds a pose, or the stabilising feedback under MPPI samples,
 * in ONE launch.  Row r follows gain trajectory g = gain_index[r]; at the START of every step t, with (qpos, qvel) the row's state
 * there (the initial row for t = 0):
 *   dx  = [ tangent_diff(qpos, qpos_ref[g, t]) ; qvel - qvel_ref[g, t] ]                                  (2 nv)
 *   u_i = ctrl[r, t, i] + sum_j gain_t[g, t, j, i] * dx_j          (j ascending, one FMA chain from 0, then one add)
 * and u is the ctrl of step t.  tangent_diff is MuJoCo's mj_differentiatePos (gym_kmanip_amd/derivatives.py tangent_diff, the same
 * branches): joints and cube position subtracted, the rotation the body-frame log of quat_ref^-1 (x) quat.  The first eight fields
 * are KRolloutIn's, with its NULL semantics; ctrl is the open-loop term.  T = gain_per_step ? nstep : 1. */
typedef struct KFeedbackIn {
  const int32_t* env_index;    /* [n] DEVICE or NULL: KRolloutIn::env_index */
  const double*  qpos;         /* [n, nq] or NULL: the named env's stored qpos */
  const double*  qvel;         /* [n, nv] or NULL */
  const double*  qacc_warm;    /* [n, nv] or NULL */
  const double*  ctrl;         /* ctrl_per_step ? [n, nstep, nu] : [n, nu], or NULL (the named env's stored ctrl, held): the open-loop
                                  term of the policy */
  const double*  qfrc_applied; /* frc_per_step ? [n, nstep, nv] : [n, nv], or NULL: KRolloutIn::qfrc_applied */
  int32_t ctrl_per_step;       /* 1: row (r, t) of ctrl belongs to step t; 0: row r is held for all steps */
  int32_t frc_per_step;        /* likewise for qfrc_applied */
  const int32_t* gain_index;   /* [n] DEVICE: row r follows gain trajectory gain_index[r]; many rows may share one (a line search
                                  over the step size, K candidates per env).  NULL = row r follows trajectory r, and then ng >= n */
  const double*  qpos_ref;     /* [ng, T, nq] the reference state BEFORE step t (record t of an earlier rollout is the state AFTER
                                  step t: the reference of step t + 1) */
  const double*  qvel_ref;     /* [ng, T, nv] */
  const double*  gain_t;       /* [ng, T, 2 nv, nu] the gain TRANSPOSED: entry (j, i) multiplies tangent component j into actuator i */
  int32_t ng;                  /* gain trajectories */
  int32_t gain_per_step;       /* 1: T = nstep, entry t acts at the start of step t; 0: T = 1, the one reference and gain are held
                                  (a regulator) */
} KFeedbackIn;
/* OUTPUTS, written at the ROW; any field may be NULL.  The first seven are KRolloutDev's. */
typedef struct KFeedbackDev {
  double*   qpos;          /* [n, nstep, nq] the state after each step */
  double*   qvel;          /* [n, nstep, nv] */
  double*   qacc_warm;     /* [n, nstep, nv] */
  uint32_t* contact_mask;  /* [n, nstep] */
  double*   reward;        /* [n, nstep] */
  uint8_t*  status;        /* [n] KRolloutDev::status, and: 1 also for a non-finite u (a non-finite reference or gain entry the row
                              uses, or an overflow); 2 also for gain_index[r] outside 0 .. ng-1: the entry is compared before it is
                              ever used as an address */
  int32_t*  steps_done;    /* [n] whole steps recorded before the row stopped; a non-finite u at step t leaves t */
  double*   ctrl;          /* [n, nstep, nu] u, the control that acted during each step, UNCLAMPED: the servos' ctrlrange /
                              forcerange act inside the sub-steps as always.  Zeros from step steps_done on, like every record */
} KFeedbackDev;
/* Everything else -- the sub-step loop, nsub == 0, the handle's solver, the trailing pass, the zero tail, n == 0 or nstep == 0 -- is
 * kmanip_rollout's.  With every gain entry zero the rows are kmanip_rollout's, bit for bit, and ctrl out is ctrl in.
 * ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  THE HANDLE IS READ ONLY.
 * ERRORS: everything kmanip_rollout refuses, a NULL qpos_ref, qvel_ref or gain_t, ng <= 0, or a NULL gain_index with ng < n return
 * nonzero with kmanip_last_error set and launch nothing.
 * OUT OF SCOPE: nonlinear policies, feedback per sub-step other than through nsub == 1 (a policy clamped to a box: kmanip_feedback_box),
 * analytic derivatives (gym_kmanip_amd/ilqr.py builds the iLQR loop from kmanip_rollout, transition_fd and this entry). */
KMANIP_API int kmanip_feedback(KHandle h, const KFeedbackIn* in, int n, int nstep, int nsub, const KFeedbackDev* out, void* stream);

/* kmanip_feedback with the policy's output clamped to a box -- the forward pass of control-limited DDP: at
 * every step boundary, after kmanip_feedback's finite-u test,
 *   u_i = min(max(ctrl[r, t, i] + sum_j gain_t[g, t, j, i] * dx_j, lo[b, i]), hi[b, i]),     b = box_per_traj ? g : 0
 * and the clamped u is what acts and what KFeedbackDev::ctrl records.  -inf / +inf leave a side open; with every bound infinite every
 * output byte is kmanip_feedback's.  A row whose box has lo_i <= hi_i false for some i (lo > hi, a NaN bound) gets status 1 and no
 * step.  Everything else, the refusals included, is kmanip_feedback's; a NULL lo or hi is refused as well.  The kernels are
 * kmanip_rollout.hip built a third time (KM_VAR_FB=2, the kmanip_boxfb_* objects): kmanip_feedback's own objects are untouched. */
typedef struct KFeedbackBoxIn { /* KFeedbackIn's fields, in its order and with its meanings, then the box */
  const int32_t* env_index;
  const double*  qpos;
  const double*  qvel;
  const double*  qacc_warm;
  const double*  ctrl;
  const double*  qfrc_applied;
  int32_t ctrl_per_step;
  int32_t frc_per_step;
  const int32_t* gain_index;
  const double*  qpos_ref;
  const double*  qvel_ref;
  const double*  gain_t;
  int32_t ng;
  int32_t gain_per_step;
  const double* lo;            /* [box_per_traj ? ng : 1, nu] DEVICE */
  const double* hi;            /* [box_per_traj ? ng : 1, nu] DEVICE */
  int32_t box_per_traj;        /* 1: gain trajectory g has its own box (row g of lo / hi); 0: one box for all */
} KFeedbackBoxIn;
KMANIP_API int kmanip_feedback_box(KHandle h, const KFeedbackBoxIn* in, int n, int nstep, int nsub, const KFeedbackDev* out, void* stream);

/* Finite-difference derivatives of ONE step at rows the caller passes, MuJoCo's mjd_transitionFD: what
 * gym_kmanip_amd/derivatives.py transition_fd assembles from two kmanip_rollout calls and torch arithmetic, with the perturbation of
 * the rows and the difference quotient inside the kernel.  The state is s = (qpos in the tangent space, qvel), 2 nv wide; the columns
 * are the inputs named by `wrt`, ALWAYS in the order qpos (nv tangent columns), qvel (nv), ctrl (nu), qfrc_applied (nv):
 * ncol = the sum of the widths of the bits set. */
#define KM_WRT_QPOS 1
#define KM_WRT_QVEL 2
#define KM_WRT_CTRL 4
#define KM_WRT_FRC  8
typedef struct KTransFdIn {
  const int32_t* env_index;    /* [n] DEVICE or NULL: KRolloutIn::env_index */
  const double*  qpos;         /* [n, nq] or NULL: the named env's stored qpos */
  const double*  qvel;         /* [n, nv] or NULL */
  const double*  qacc_warm;    /* [n, nv] or NULL: the nominal rows' warm start, and the BASE of the perturbed rows' */
  const double*  ctrl;         /* [n, nu] or NULL: the named env's stored ctrl, used exactly as given / stored */
  const double*  qfrc_applied; /* [n, nv] or NULL: the named env's row of a bound applied force, none if nothing is bound (a
                                  differentiated force that nobody gave and nothing binds is rows of zeros) */
  int32_t wrt;                 /* KM_WRT_* bits */
  double  eps;                 /* the perturbation: +-eps on one entry; cube-rotation column k multiplies the quaternion on the right
                                  by [cos(eps / 2), +-sin(eps / 2) e_k] (the body-frame convention of qvel's angular part) */
  double  warm_offset;         /* added on every dof to the base of the perturbed rows' first warm start (derivatives.py transition_fd:
                                  THE WARM START); 0 = the plain warm start */
} KTransFdIn;
/* OUTPUTS; any field may be NULL unless stated otherwise. */
typedef struct KTransFdDev {
  double*   qpos;            /* [n, nq] the NOMINAL rows one step on: exactly what kmanip_rollout(.., nstep = 1, nsub) writes */
  double*   qvel;            /* [n, nv] */
  double*   qacc_warm;       /* [n, nv]; must be given when KTransFdIn::qacc_warm is NULL and wrt != 0: it is then the warm-start base
                                of the perturbed rows, and the library allocates nothing */
  uint32_t* contact_mask;    /* [n] */
  uint8_t*  status;          /* [n] KRolloutDev::status of the nominal rows */
  double*   deriv_t;         /* [n, ncol, 2 nv] entry (r, c, i) = d s'_i / d input_c, TRANSPOSED (the column is the slow index: the lanes
                                of a group write one contiguous run of 2 nv doubles per column).  Must be given when wrt != 0 */
  uint8_t*  status_cols;     /* [n, ncol] the larger KRolloutDev::status of the column's +eps and -eps rows; nonzero: the column is
                                zeros, not a derivative */
  uint32_t* contact_mask_fd; /* [n, ncol, 2] the contact mask after the step of the +eps and of the -eps row (0 for a row that stopped);
                                the trailing kinematics + collision pass of the perturbed rows is skipped when this is NULL */
} KTransFdDev;
/* PER ROW the arithmetic is derivatives.py transition_fd's, operation for operation: the perturbed rows start their first sub-step at
 * (KTransFdIn::qacc_warm if given, else the nominal row's qacc_warm after its step) + warm_offset; the sub-step loop is kmanip_rollout's
 * (nsub == 0: the model's n_sub_steps; the handle's solver; the same divergence tests); entry (r, c, .) =
 * [tangent_diff(qpos+, qpos-) ; qvel+ - qvel-] / (2.0 * eps), a division.  A column whose +eps or -eps row stops (status 1) or whose
 * row names an env outside the handle (status 2: compared before it is ever used as an address) is zeros, with its status_cols entry.
 * TWO kernel launches on `stream`, ordered by it: the nominal rows through kmanip_rollout's kernel (nstep = 1), then the n * ncol
 * column pairs.  No allocation, no synchronisation, no host copy.  THE HANDLE IS READ ONLY.  n == 0 succeeds and does nothing;
 * wrt == 0 does the nominal launch only.
 * ERRORS: a NULL handle, `in` or `out`, n < 0, nsub < 0, n > num_envs with a NULL env_index, wrt bits outside 15, eps not finite or
 * <= 0, a non-finite warm_offset, wrt != 0 with a NULL deriv_t, wrt != 0 with both KTransFdIn::qacc_warm and KTransFdDev::qacc_warm
 * NULL, or 2 * ncol * n beyond int return nonzero with kmanip_last_error set, launch nothing and leave the outputs untouched.
 * OUT OF SCOPE: derivatives of kmanip_forward, of more than one step, analytic derivatives, one-sided differences. */
KMANIP_API int kmanip_transition_fd(KHandle h, const KTransFdIn* in, int n, int nsub, const KTransFdDev* out, void* stream);

/* The backward pass of iLQR -- the Riccati recursion of gym_kmanip_amd/ilqr.py backward_pass -- for n independent problems of T steps
 * in ONE launch: it reads kmanip_transition_fd's deriv_t as it lies in memory and writes KFeedbackIn::gain_t's
 * layout, so that neither side copies or transposes.  nx = 2 nv and nu are the handle's model's; n is the number of PROBLEMS and has
 * nothing to do with num_envs.  With Vx = lx[T], Vxx = lxx[T], for t = T-1 .. 0 (A, B the step's, ' the transpose):
 *   Qx  = lx[t] + A' Vx              Qu  = lu[t] + B' Vx
 *   Qxx = lxx[t] + A' Vxx A          Quu = luu[t] + B' Vxx B          Qux = B' Vxx A
 *   k = -(Quu + reg I)^-1 Qu         K = -(Quu + reg I)^-1 Qux        (Cholesky of Quu + reg I, its lower triangle)
 *   Vx  = Qx + K' (Quu k + Qu) + Qux' k                               (Quu here WITHOUT reg)
 *   Vxx = Qxx + K' Quu K + K' Qux + Qux' K;   Vxx = 0.5 (Vxx + Vxx')
 *   dv[0] += k . Qu                  dv[1] += 0.5 k . (Quu k)
 * backward_pass's formulas; the sums are ordered differently and contracted to FMAs, nothing else.  No cross term lux. */
typedef struct KLqrIn {
  const double* a_t;        /* block (e, t) at a_t + (e*T + t) * a_stride: [nx, nx], entry (j, i) = A[i][j] (TRANSPOSED, rows contiguous) */
  const double* b_t;        /* block (e, t) at b_t + (e*T + t) * b_stride: [nu, nx], entry (j, i) = B[i][j] */
  int64_t a_stride, b_stride; /* in doubles; 0 = dense (nx*nx, nu*nx).  deriv_t of kmanip_transition_fd over the n*T rows e*T + t with
                                 wrt = qpos|qvel|ctrl is both: a_t = deriv_t, b_t = deriv_t + nx*nx, both strides (nx + nu) * nx */
  const double* lx;         /* [n, T+1, nx]; entry T is the final cost's */
  const double* lu;         /* [n, T, nu] */
  const double* lxx;        /* [lxx_per_env ? n : 1, T+1, nx, nx], symmetric (not checked) */
  const double* luu;        /* [luu_per_env ? n : 1, T, nu, nu], symmetric (not checked; the factorisation reads one triangle) */
  int32_t lxx_per_env, luu_per_env;
  const double* reg;        /* [n] or NULL = 0 */
} KLqrIn;
typedef struct KLqrDev {    /* any field may be NULL */
  double*  k;               /* [n, T, nu] */
  double*  gain_t;          /* [n, T, nx, nu]: KFeedbackIn::gain_t's layout, a trajectory per problem */
  double*  dv;              /* [n, 2] */
  uint8_t* status;          /* [n] */
  int32_t* fail_step;       /* [n] */
} KLqrDev;
/* STATUS per problem: 0 and fail_step -1 when every step factorised.  A problem FAILS at step t when a pivot of the Cholesky
 * factorisation is not > 0 or not finite -- an indefinite Quu + reg I, or a NaN / inf upstream of it -- or when an entry of the
 * step's k or K is not finite (a NaN in A or lu reaches the right-hand sides, not Quu): the problem stops, status 1, fail_step t,
 * and ALL of its k, gain_t and dv entries are zeros, those of the steps already done included.  (A NaN in lx[t] or lxx[t] alone
 * reaches neither at step t: it fails step t - 1, and at t = 0 it reaches nothing that is returned.)  The other problems are unaffected; a problem's result does not depend on n or on its place among the problems.
 * ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  THE HANDLE IS READ ONLY (it gives
 * the device, nx and nu).  n == 0 or T == 0 succeeds and launches nothing (the fields of `in` are then not looked at).
 * ERRORS: a NULL handle, `in` or `out`, a NULL a_t, b_t, lx, lu, lxx or luu, n < 0 or T < 0, a nonzero stride smaller than its
 * block, or n * T beyond int return nonzero with kmanip_last_error set, launch nothing and leave the outputs untouched.
 * OUT OF SCOPE: a cross term lux, second-order dynamics terms (DDP), nx /
 * nu other than the handle's model's, the cost's derivatives. */
KMANIP_API int kmanip_lqr_backward(KHandle h, const KLqrIn* in, int n, int T, const KLqrDev* out, void* stream);

/* The backward pass of CONTROL-LIMITED DDP (Tassa, Mansard, Todorov, ICRA 2014): kmanip_lqr_backward with a box
 * lo <= u_t + du <= hi on the controls, gym_kmanip_amd/ilqr.py backward_pass_box, in ONE launch.  Qx, Qu, Qxx, Quu, Qux as above; with
 * H = Quu + reg I, bl = lo - u_t, bh = hi - u_t the step solves   min_d 0.5 d'H d + Qu'd,  bl <= d <= bh   by projected Newton steps:
 *   d = clip(0, bl, bh);  repeat:
 *     g = Qu + H d;  c = { i : d_i == bl_i and g_i > 0 } u { i : d_i == bh_i and g_i < 0 }  (the clamped set; the rest is free)
 *     CONVERGED if the last step was a full one (step 1) that the clip left alone, and c is the set that step was factorised for
 *     H_ff = L L' (Cholesky; row and column i of H replaced by the unit row for i in c), only when c changed
 *     CONVERGED if every actuator is clamped
 *     s_f = -H_ff^-1 g_f, s_c = 0;  sg = s . g;  CONVERGED if sg >= 0 (an exact minimiser of the face: nothing left to descend)
 *     step a = 1, 0.6, 0.36, ..: the first with  [v(clip(d + a s)) - v(d)] / (a sg) >= 0.1;  d = clip(d + a s)
 * (Armijo 0.1, step factor 0.6, at most 100 iterations: the paper's constants.)  No gradient threshold enters: the rule compares
 * sets and steps, so it is scale-free.  Then k = d, K_f = -H_ff^-1 Qux_f, the rows of K at the clamped actuators EXACT ZEROS, and Vx,
 * Vxx, dv by kmanip_lqr_backward's formulas with these k and K (Quu without reg). */
typedef struct KLqrBoxIn {
  KLqrIn lqr;               /* kmanip_lqr_backward's inputs */
  const double* u;          /* [n, T, nu] the nominal controls */
  const double* lo;         /* [box_per_env ? n : 1, nu]; -inf = unbounded below */
  const double* hi;         /* [box_per_env ? n : 1, nu]; +inf = unbounded above */
  int32_t box_per_env;
} KLqrBoxIn;
typedef struct KLqrBoxDev { /* any field may be NULL */
  KLqrDev   lqr;            /* kmanip_lqr_backward's outputs */
  uint32_t* clamped;        /* [n, T] bit i set: actuator i ended step t's QP on a bound (clamped) */
  int32_t*  qp_iters;       /* [n, T] the projected-Newton steps step t's QP took */
} KLqrBoxDev;
/* STATUS per problem, with kmanip_lqr_backward's rule (the problem stops, fail_step t, ALL of its k, gain_t, dv, clamped and qp_iters
 * entries zeros): 1 when a pivot of a free block's factorisation is not > 0 or not finite, when an entry of the step's k or K (or
 * the step's descent s . g) is not finite, or when the step's box has bl_i <= bh_i false for some i -- lo > hi or a NaN bound (at the
 * first step solved, t = T - 1), a non-finite u_t; 3 when a step's QP reached the iteration cap, or one of its line searches ran out
 * of its 100 trials (0.6^100 < 1e-22: the paper's smallest step).  Every loop of the kernel has such a cap.
 * With every bound infinite the result is kmanip_lqr_backward's to rounding (the solve is the same factorisation; qp_iters is 1).
 * ONE kernel launch, asynchronous on `stream`; THE HANDLE IS READ ONLY; n == 0 or T == 0 succeeds and launches nothing.
 * ERRORS: everything kmanip_lqr_backward refuses, and a NULL u, lo or hi.
 * OUT OF SCOPE: per-step bounds, a cross term lux, a warm start of the QP from an earlier pass, forcerange-aware planning. */
KMANIP_API int kmanip_lqr_backward_box(KHandle h, const KLqrBoxIn* in, int n, int T, const KLqrBoxDev* out, void* stream);

/* The ADJOINT sweep of a rollout -- the first-order use of the step Jacobians (gym_kmanip_amd/derivatives.py
 * adjoint_pass is the definition, gym_kmanip_amd/grad.py builds rollout_grad, rollout_jacobian and diff_rollout on it): the gradient
 * of a scalar loss on a trajectory with respect to the controls and the initial state, for n problems of T steps and m >= 1
 * COTANGENT VECTORS per problem in ONE launch.  Row r = e * m + j carries vector j through the dynamics of problem e, which are
 * addressed exactly as in KLqrIn (a_t, b_t, a_stride, b_stride, transposed blocks: kmanip_transition_fd's deriv_t is read where it
 * lies, and a deriv_t that also carries the qfrc_applied columns works through the stride alone).  With gx the loss's direct partials
 * with respect to the tangent state x_t, gu those with respect to u_t, lam[T] = gx[T], for t = T-1 .. 0:
 *   mu[t]_i  = gu[t]_i + sum_k B_t[k][i] lam[t+1]_k
 *   lam[t]_j = gx[t]_j + sum_k A_t[k][j] lam[t+1]_k + sum_i K_t[i][j] mu[t]_i         (the last sum only when gains are given)
 * lam[0] is the gradient with respect to the initial tangent state, mu[t] the gradient with respect to the control that ACTED at
 * step t -- the gradient with respect to ctrl of an open-loop rollout, and with respect to the open-loop term of kmanip_feedback's
 * policy u = ctrl + K dx.  The gradient with respect to K_t is the outer product mu[t] (x) dx_t: torch arithmetic for the caller.
 * THE ORDER OF EVERY SUM: one FMA chain from 0 over k ascending, for lam continued over i ascending, then ONE add of the direct term
 * (gx or gu; a NULL gu adds 0.0).  A row's result does not depend on n, on m or on the row's place; with every gain entry zero the
 * bytes are the open-loop ones.
 * THE ONE APPROXIMATION: with gains, dx_t = tangent_diff(x_t, ref_t) is taken as linear in the state (the log map's Jacobian at the
 * cube's rotation as the identity, QuadraticCost's Gauss-Newton habit): exact when the cube-rotation columns of K (those rows of gain_t) are zero. */
typedef struct KAdjointIn {
  const double* a_t;        /* KLqrIn::a_t: block (e, t) at a_t + (e*T + t) * a_stride, [nx, nx] TRANSPOSED */
  const double* b_t;        /* KLqrIn::b_t: block (e, t) at b_t + (e*T + t) * b_stride, [nu, nx] */
  int64_t a_stride, b_stride; /* in doubles; 0 = dense (nx*nx, nu*nx) */
  const double* gx;         /* [n*m, T+1, nx]; entry 0 belongs to x_0, entry T to the final state */
  const double* gu;         /* [n*m, T, nu], or NULL = zeros */
  const double* gain_t;     /* [n, T, nx, nu]: KFeedbackIn::gain_t's layout, a trajectory per problem; NULL = open loop */
} KAdjointIn;
typedef struct KAdjointDev { /* either field may be NULL */
  double* lam;              /* [n*m, T+1, nx] */
  double* mu;               /* [n*m, T, nu] */
} KAdjointDev;
/* NO STATUS: nothing is factorised, and a non-finite input propagates as IEEE arithmetic propagates it, into the outputs of the rows
 * that read it only (a NaN in one row's gx stays in that row; one in A_t reaches every row of its problem).
 * ONE kernel launch, asynchronous on `stream`: no allocation, no synchronisation, no host copy.  THE HANDLE IS READ ONLY (it gives
 * the device, nx and nu).  n == 0, T == 0 or m == 0 succeeds and launches nothing (the fields of `in` are then not looked at).
 * ERRORS: a NULL handle, `in` or `out`, a NULL a_t, b_t or gx, n < 0, T < 0 or m < 0, a nonzero stride smaller than its block, or
 * n * m * T beyond int return nonzero with kmanip_last_error set, launch nothing and leave the outputs untouched.
 * OUT OF SCOPE: gradients through the clamped policy of kmanip_feedback_box, with respect to qfrc_applied, the model's parameters or
 * the warm start (the solver's starting point, not a state), second-order terms, the gradient with respect to the references of the
 * policy (-K' mu: one line for the caller), analytic step derivatives. */
KMANIP_API int kmanip_adjoint(KHandle h, const KAdjointIn* in, int n, int T, int m, const KAdjointDev* out, void* stream);

/* KManipEnv.reset(seed=...) (env_base.py:219-220): re-key the cube-spawn stream.  restart_episodes != 0 also rewinds every
 * env's episode counter so that the next kmanip_reset draws episode 0 of the new seed (reset(seed=s) is then reproducible). */
KMANIP_API int kmanip_set_seed(KHandle h, uint64_t seed, int restart_episodes);

/* Per-env diagnostics of the last kmanip_step (HOST pointers, may be NULL):
 * contact_mask uint32 (KM_CON_* bits, from the trailing mj_step1), ik_nfev int32[num_envs, 2],
 * ik_status int32[num_envs, 2]. Synchronous. */
KMANIP_API int kmanip_get_diag(KHandle h, uint32_t* contact_mask, int32_t* ik_nfev, int32_t* ik_status);

/* Kernel timing with HIP events recorded on the launch stream (bench.py roofline leg).  While enabled, every kmanip_step
 * records an event before and after k_step and one more after the bound in-step render (or after the first kmanip_render_rgb[_multi]
 * / kmanip_render_labels_multi call that follows the step: the camera observations of a *Vision id), into a ring of `KM_TIMING_SLOTS` steps (an event record
 * costs the stream about 5 us).  kmanip_timing_summary synchronises the device and returns the summed durations in milliseconds of
 * k_step and of the step's render (kmanip_bind_step_depth's or the RGB render called after the step, 0 without one) over the
 * recorded steps, then clears the ring.  *ik_ms_sum is always 0: before_step runs inside k_step, and the argument is kept for ABI
 * compatibility.  Any output pointer may be NULL.
 * `enable` = k > 1 records every k-th step only (the first step after the call, then every k-th): the events' own cost -- the ~5 us
 * above, 1 % of a 4096-env step -- then falls on one step in k, and the averages are over the sampled steps (`*nsteps` = their count). */
#define KM_TIMING_SLOTS 1024
KMANIP_API int kmanip_enable_timing(KHandle h, int enable);
KMANIP_API int kmanip_timing_summary(KHandle h, double* ik_ms_sum, double* dyn_ms_sum, double* render_ms_sum, int32_t* nsteps);

/* nsteps control steps in ONE launch, for callers that already hold the next nsteps actions of every env (action-chunking
 * policies such as ACT, scripted / replayed action streams): exactly the result of nsteps consecutive kmanip_step calls,
 * with act_dev float[nsteps, num_envs, act_dim], obs_dev double[nsteps, num_envs, obs_dim], reward_dev double[nsteps,
 * num_envs], done_dev uint8[nsteps, num_envs].  Without a launch boundary per step the waves do not wait for the
 * batch's slowest env at every step, so throughput follows the mean wave rather than the slowest one.  A bound applied force
 * (kmanip_bind_applied_force) is read once, at the launch: the same row acts in every step of the chunk. */
KMANIP_API int kmanip_step_chunk(KHandle h, int nsteps, const float* act_dev, double* obs_dev, double* reward_dev,
                      uint8_t* done_dev, void* stream);

/* Standalone batched IK (ik_mujoco.ik, reference ik_mujoco.py:100-155) for parity tests:
 * qpos HOST double[n, nq] (in: current; out: qpos after the IK's last evaluation),
 * goal_pos double[n,3], goal_quat double[n,4] (wxyz), arm 0/1; q_out double[n, arm_nq]
 * (the clipped result.x that the reference writes into ctrl). Synchronous. */
KMANIP_API int kmanip_ik(KHandle h, int arm, int n, double* qpos, const double* goal_pos,
              const double* goal_quat, double* q_out, int32_t* nfev, int32_t* status);

/* ik_res / ik_jac (reference ik_mujoco.py:20-53 / :56-97) as the device IK evaluates them, at x = qpos[q_mask] with
 * q_pos_prev = x, for parity tests: qpos HOST double[n, nq], goal_pos [n,3], goal_quat [n,4] (wxyz);
 * res double[n, 6 + 2*arm_nq], jac double[n, (6 + 2*arm_nq) x arm_nq] row-major.  Synchronous. */
KMANIP_API int kmanip_ik_eval(KHandle h, int arm, int n, const double* qpos, const double* goal_pos,
                   const double* goal_quat, double* res, double* jac);

/* Replaces KManipEnvSim.k_render (env_sim.py:187-188) / the camera branch of get_observation
 * (env_sim.py:140-145) for the gripper cameras, as BASELINE.json config 5 defines it: a height x width
 * float32 DEPTH image (metres along the optical axis) of every env's current state.
 * depth_dev: float[num_envs, height, width] device memory owned by the caller. */
KMANIP_API int kmanip_render_depth(KHandle h, int cam, int height, int width, float* depth_dev, void* stream);   /* (link capsules: only after kmanip_set_depth_links) */

/* The same cameras as uint8 RGB, what dm_control's physics.render(height, width, camera_id) returns for the camera
 * observations of the *Vision env ids (env_sim.py:140-145; shapes env_base.py:140-146, cameras __init__.py:157-161) and for
 * KManipEnv.render() (env_base.py:215-217, the `top` camera): rgb_dev uint8[num_envs, height, width, 3], caller-owned
 * device memory.  Lambert shading of the surrogate scene under the reference's lights (scene.xml:8-13). */
KMANIP_API int kmanip_render_rgb(KHandle h, int cam, int height, int width, uint8_t* rgb_dev, void* stream);
/* ncam (<= KM_MAX_CAMS) of those images in ONE launch: the whole camera branch of a *Vision observation (head 480 x 640 + grip
 * 40 x 60 per arm: env_base.py:140-146) costs the step's stream one launch instead of one per camera.  cams / heights / widths /
 * rgb_dev are HOST arrays of ncam entries; rgb_dev[i] is device memory uint8[num_envs, heights[i], widths[i], 3]. */
KMANIP_API int kmanip_render_rgb_multi(KHandle h, int ncam, const int* cams, const int* heights, const int* widths, uint8_t* const* rgb_dev,
                            void* stream);

/* Per-pixel segmentation labels of the same ray cast: the class of what the pixel's ray hits first.
 * 0..2 are the ray caster's materials; a robot pixel carries the arm of the finger sphere that was hit (sphere s belongs to arm a
 * when sphere_link[s] is an ancestor-or-self of arm_site_link[a] or of one of arm_grip_id[a][*]; gym_kmanip_amd/model.py
 * sphere_arm) or, while the handle has link capsules (kmanip_set_render_links), the `label` of the capsule that was hit.  A label depends on geometry only: colours and lights (KM_VP_*) never change it, the per-env camera offset moves it
 * exactly as it moves the RGB image. */
enum { KM_SEG_BACKGROUND = 0, KM_SEG_TABLE = 1, KM_SEG_CUBE = 2, KM_SEG_ROBOT_R = 3, KM_SEG_ROBOT_L = 4, KM_SEG_N = 5 };
/* ncam jobs in ONE launch.  seg_dev[i]: device uint8[num_envs, heights[i], widths[i]] (KM_SEG_* values) or NULL;
 * rgb_dev[i]: device uint8[num_envs, heights[i], widths[i], 3] or NULL; rgb_dev itself may be NULL (labels only).  A job with
 * neither is an error.  The RGB bytes are those kmanip_render_rgb_multi writes.  Snapshots (kmanip_set_render_source), visual
 * parameters and kmanip_enable_timing are honoured as by kmanip_render_rgb_multi. */
KMANIP_API int kmanip_render_labels_multi(KHandle h, int ncam, const int* cams, const int* heights, const int* widths,
                               uint8_t* const* rgb_dev, uint8_t* const* seg_dev, void* stream);
KMANIP_API int kmanip_render_seg(KHandle h, int cam, int height, int width, uint8_t* seg_dev, void* stream);   /* one camera, labels only */

/* Link capsules: an opt-in, per-handle list of capsules -- a segment fixed in a link's frame, with a
 * radius -- that the RGB and label renders draw as robot material (KM_VP_ROBOT_RGB, shaded like the finger spheres, under the
 * env's light terms and camera offset) and label with `label`.  While a handle has a list, kmanip_render_rgb[_multi],
 * kmanip_render_seg and kmanip_render_labels_multi launch k_render_links instead of k_render_rgb / k_render_labels; snapshots,
 * visual parameters and kmanip_enable_timing's render leg are honoured as before.  With no list (the default) every launch is
 * exactly what it was: the same kernels, the same bytes.  Objects are tested in the order table, cube, spheres, capsules in
 * list order, and a later object wins only where it is strictly nearer.  Only a ray's entry point counts: a camera inside a
 * capsule sees through it, as it does through a sphere.  Depth is a switch of its own: kmanip_render_depth and kmanip_bind_step_depth
 * draw the scene without capsules until kmanip_set_depth_links turns them on.  The capsules are drawn only; the physics never reads them.
 * gym_kmanip_amd/model.py link_capsules builds the default list (joint-to-joint capsules along both arms plus the fingers). */
#define KM_MAX_LINK_CAPSULES 24
typedef struct KLinkCapsule {
  int32_t  link;      /* 0 .. nlink-1: the frame p0 / seg are given in                      */
  int32_t  label;     /* KM_SEG_ROBOT_R or KM_SEG_ROBOT_L: what a pixel of it is labelled   */
  uint32_t cam_mask;  /* bit KM_CAM_*: drawn by that camera                                 */
  int32_t  pad_;
  double   p0[3], seg[3];   /* axis from p0 to p0 + seg, link frame; seg = 0 is a sphere    */
  double   radius;          /* metres, > 0                                                  */
} KLinkCapsule;
/* caps: HOST array of n entries; n = 0 or caps == NULL with n = 0: no list (the default kernels again).  Validated first
 * (0 <= n <= KM_MAX_LINK_CAPSULES, link in range, label KM_SEG_ROBOT_R / _L, radius finite and > 0, p0 and seg finite): a bad list
 * returns nonzero, sets kmanip_last_error and leaves the handle as it was.  Synchronous (the whole device is idle when it
 * returns); the list is read when a render LAUNCHES. */
KMANIP_API int kmanip_set_render_links(KHandle h, int n, const KLinkCapsule* caps);
/* The list in force: *n entries into caps, a HOST array with room for KM_MAX_LINK_CAPSULES (caps may be NULL: the count only). */
KMANIP_API int kmanip_get_render_links(KHandle h, int* n, KLinkCapsule* caps);

/* Depth renders draw the handle's capsule list too (default 0: they never do).  A per-handle flag, separate
 * from the list and surviving its changes: while it is on AND the list is not empty, kmanip_render_depth and the in-step render of
 * kmanip_bind_step_depth launch k_render_depth_links -- the float64 depth ray cast with the capsules tested after the spheres, in
 * list order, by the ray test above in float64; `label` is ignored, cam_mask honoured -- and otherwise exactly what they launch
 * without it: the same kernels, the same bytes.  Snapshots, both visual-parameter modes (the per-env camera offset and its episode
 * draw) and kmanip_enable_timing's render leg are honoured as kmanip_render_depth honours them.  Synchronous, like
 * kmanip_set_render_links; the flag and the list are read when a render LAUNCHES. */
KMANIP_API int kmanip_set_depth_links(KHandle h, int on);
KMANIP_API int kmanip_get_depth_links(KHandle h, int* on);

/* Camera geometry.  MuJoCo's data.cam_xpos / cam_xmat of camera `cam`, per env, as the renders build it:
 * pose_dev DEVICE double[num_envs, 12] = origin (3), then the 3x3 row-major matrix whose COLUMNS are the camera's x (right),
 * y (up), z (the camera looks along -z) axes in the world frame.  Honours kmanip_set_render_source (a snapshot's qpos and, in
 * visual ranges mode, its episode counters) and the per-env camera offset in both visual-parameter modes, exactly as
 * kmanip_render_depth does.  Asynchronous on `stream`. */
KMANIP_API int kmanip_get_camera_poses(KHandle h, int cam, double* pose_dev, void* stream);

/* The point cloud of a depth image: the back-projection of what kmanip_render_depth draws on this handle at this moment (the
 * surrogate scene, plus the capsule list while kmanip_set_depth_links is on and the list is not empty), by the same float64 ray
 * cast.  Pixel (r, c) of a height x width image has the ray direction d = x dx + y dy - z in the camera's axes, with
 * dx = (c + 0.5 - width/2) / f, dy = -(r + 0.5 - height/2) / f, f = (height/2) / tan(fovy/2); D is the pixel's depth in float64 (the
 * nearest hit along the optical axis, clipped to [cam_znear, cam_zfar], no hit = cam_zfar).  Written per pixel:
 *   frame KM_POINTS_CAMERA: (float)(D dx), (float)(D dy), (float)(-D)   (the camera's own axes: x right, y up, looking along -z)
 *   frame KM_POINTS_WORLD : (float)(o + D d), evaluated in float64 and rounded once (o, x, y, z: kmanip_get_camera_poses)
 *   depth_dev, unless NULL: (float)D, the image kmanip_render_depth writes, from the same launch
 * A pixel without a hit is the point on the far plane: mask with depth >= cam_zfar.
 * xyz_dev DEVICE float[num_envs, height, width, 3]; depth_dev DEVICE float[num_envs, height, width] or NULL.  Snapshots, both
 * visual-parameter modes and kmanip_enable_timing are honoured as by kmanip_render_depth.  A NULL handle or xyz_dev, a camera the
 * model does not have, height / width < 1 or an unknown frame return nonzero with kmanip_last_error set and launch nothing. */
enum { KM_POINTS_CAMERA = 0, KM_POINTS_WORLD = 1 };
KMANIP_API int kmanip_render_points(KHandle h, int cam, int height, int width, int frame,
                                    float* xyz_dev, float* depth_dev, void* stream);

/* Rendering BEHIND the steps (a data-generation loop whose policy does not look at the images: the reference's scripted heuristic,
 * examples/2_synthetic_data.py:28-41, logs them and acts on the state).  A render reads nothing of the state but qpos (and, in
 * visual ranges mode, the episode counters the colour / light / camera draw uses: kmanip_set_visual_param_ranges):
 * kmanip_snapshot_render_state copies them into snapshot `slot` (0 or 1) on `stream` -- the step's stream, after the step whose
 * images are wanted -- and kmanip_set_render_source(h, slot) makes the kmanip_render_* calls that follow read that copy
 * (-1: the live state again, the default; host-side switch, not stream-ordered).  The caller can then issue the render on a
 * SECOND stream while the next kmanip_step runs on the first: the render's workgroups take the SIMDs the step's early-finishing
 * waves free (one 2048-env step + head and grip images: 0.96 ms in sequence, 0.67 ms this way; gym_kmanip_amd/pipeline.py
 * RenderBehind).  Ordering is the caller's: the render stream waits for the copy (an event), and a slot is not overwritten before
 * the render that reads it has finished.  kmanip_bind_step_depth's in-step render always reads the live state. */
KMANIP_API int kmanip_snapshot_render_state(KHandle h, int slot, void* stream);
KMANIP_API int kmanip_set_render_source(KHandle h, int slot);

/* BASELINE config 5 ("64x64 gripper-cam depth render in the step"): bind a caller-owned device buffer
 * float[num_envs, height, width]; every kmanip_step then ends by rendering camera `cam` of the state it produced into it,
 * on the step's stream (one C call per control step).  depth_dev == NULL unbinds.  The render draws the handle's link capsules
 * while kmanip_set_depth_links is on and a list is set, as kmanip_render_depth does. */
KMANIP_API int kmanip_bind_step_depth(KHandle h, int cam, int height, int width, float* depth_dev);

/* The scripted data-generation policy of reference examples/2_synthetic_data.py:28-41, for every env, on device:
 * act_dev float[num_envs, act_dim] arrives holding action_space.sample() (the caller draws it) and leaves with its
 * eer_pos columns overwritten by the unit vector from the right end-effector site to the cube centre
 * (cube_pos - site("eer_site_pos").xpos, normalised), evaluated at the env's current state.  The reference
 * stores that vector as float64 in the action dict; the flat action buffer is float32 (ACT_DTYPE).
 * Returns an error for env ids without an eer_pos action (the *QPos ids). */
KMANIP_API int kmanip_scripted_action(KHandle h, float* act_dev, void* stream);

/* action_space.sample() for every env, on device -- what the reference's rollout loops feed env.step with
 * (examples/2_log_with_h5py.py:22-26, 3_save_to_video.py:20-27; spaces env_base.py:151-188: every key a Box(-1, 1, float32)):
 * act_dev float[num_envs, act_dim] is filled with U[-1, 1) float32 from a counter-based stream, Philox4x32-10 keyed by the
 * handle's seed with counter (global env id, episode, step): the action of an env at a given (episode, step) does not depend
 * on the shard layout or on what was drawn before, and the CPU oracle draws identical bits (SURVEY 8d's synthetic inputs).
 * `ahead` >= 0 draws the action the env will need `ahead` control steps from now, assuming TimeLimit-only episodes (the
 * reference never terminates early), so the next K actions can be laid out before stepping. */
KMANIP_API int kmanip_sample_action(KHandle h, float* act_dev, int ahead, void* stream);

/* Per-env physics parameters (domain randomisation).  Storage is double[KM_EP_N][num_envs], struct-of-arrays
 * like the state: element (k, env) at k * num_envs + env.  Env e with parameters p behaves exactly like a handle whose KModelDesc is
 * the compiled one with these fields and their derived constants replaced (gym_kmanip_amd/model.py with_env_params):
 *   KM_EP_CUBE_MASS          cube mass m_e, kg; uniform-density box of unchanged size: cube_inertia[k] * (m_e / cube_mass),
 *                            cube_invweight0 and meaninertia follow
 *   KM_EP_CUBE_FRICTION      tangential friction of the pairs with the cube (con_cube_friction[0]); torsional / rolling unchanged
 *   KM_EP_CUBE_FRICTIONLOSS  friction loss of the cube's free joint (its rows exist only while the value is > 0)
 *   KM_EP_KP_SCALE           multiplier on every position servo's kp (ctrlrange / forcerange unchanged)
 * Nothing else (geometry, gravity, spawn box, cameras) is per env. */
enum { KM_EP_CUBE_MASS = 0, KM_EP_CUBE_FRICTION = 1, KM_EP_CUBE_FRICTIONLOSS = 2, KM_EP_KP_SCALE = 3, KM_EP_N = 4 };

/* Explicit values: params_dev DEVICE double[KM_EP_N][num_envs], read once `stream` has produced it; switches ranges mode off.
 * Synchronous: returns after the whole device is idle and the values are copied (a step in flight on any stream finishes first).  The values are
 * validated on the device first (mass > 0, friction >= 0, frictionloss >= 0, kp_scale > 0, all finite; one flag read back per
 * call, never per step): a bad value returns nonzero and leaves the handle unchanged.  params_dev == NULL returns to the compiled
 * model: the default kernels, bit-identical to a handle that never had parameters. */
KMANIP_API int kmanip_set_env_params(KHandle h, const double* params_dev, void* stream);
/* The values in force into DEVICE double[KM_EP_N][num_envs] on `stream` (the compiled model's when none are set); in ranges mode,
 * after a reset, the values drawn for the env's current episode. */
KMANIP_API int kmanip_get_env_params(KHandle h, double* params_dev, void* stream);
/* Ranges mode: lo / hi HOST double[KM_EP_N].  From then on every reset of env e -- kmanip_reset's mask or the auto-reset inside
 * kmanip_step / kmanip_step_chunk -- draws p_k = lo[k] + (hi[k] - lo[k]) * u_k (product rounded before the sum), u_k a 53-bit
 * uniform from Philox4x32-10 keyed by the seed with counter (global env id lo, hi, episode, KM_EP_CTR3 + k / 2): words (0, 1)
 * of the block for even k, (2, 3) for odd k; `episode` is the one the reset's cube spawn uses.  lo == hi pins a parameter.  Envs
 * keep their current values until their next reset.  lo > hi or a value outside the limits above is refused (handle unchanged);
 * NULL, NULL turns ranges mode off and keeps the values in force.  Synchronous. */
#define KM_EP_CTR3 2u
KMANIP_API int kmanip_set_env_param_ranges(KHandle h, const double* lo, const double* hi);

/* Finite-difference derivatives of ONE step with respect to the per-env physics parameters, at rows the caller passes (DESIGN.md
 * section 42): P = d s' / d p, s = (qpos in the tangent space, qvel) as in kmanip_transition_fd, whose sibling this is.  The columns
 * are the parameters named by `wrt` (bit k = KM_EP_* k) in ascending k: npar = the number of bits set.  The +e and -e rows of a
 * column are stepped side by side in one wave with the parameter replaced in the kernel's workspace, and the quotient is formed there:
 * no perturbed parameter and no perturbed state reaches memory, and the handle's parameters are not touched. */
typedef struct KParamFdIn {
  const int32_t* env_index;    /* [n] DEVICE or NULL: KRolloutIn::env_index */
  const double*  qpos;         /* [n, nq] or NULL: the named env's stored qpos */
  const double*  qvel;         /* [n, nv] or NULL */
  const double*  qacc_warm;    /* [n, nv] or NULL: the named env's stored warm start; the BASE of both rows' first sub-step */
  const double*  ctrl;         /* [n, nu] or NULL: the named env's stored ctrl, used exactly as given / stored */
  const double*  qfrc_applied; /* [n, nv] or NULL: the named env's row of a bound applied force, none if nothing is bound */
  const double*  params;       /* [n, KM_EP_N] DEVICE or NULL: row r's parameters (ROW-major, unlike the handle's storage).  NULL: the
                                  values in force for env env_index[r] (in ranges mode the drawn ones); on a handle without per-env
                                  parameters the compiled model's */
  int32_t wrt;                 /* bit k = differentiate KM_EP_* k */
  double  eps[KM_EP_N];        /* the perturbation of each parameter (read for the selected ones only) */
  int32_t eps_relative;        /* 1: e = fl(eps[k] * p_k); 0: e = eps[k] */
  double  warm_offset;         /* added on every dof to the base of both rows' first warm start (KTransFdIn::warm_offset) */
} KParamFdIn;
/* OUTPUTS; status_cols and contact_mask_fd may be NULL. */
typedef struct KParamFdDev {
  double*   deriv_t;         /* [n, npar, 2 nv] entry (r, c, i) = d s'_i / d p_c, TRANSPOSED like KTransFdDev::deriv_t.  Must be given */
  uint8_t*  status_cols;     /* [n, npar] 0 a derivative; 1 the + or - row stopped (KRolloutDev::status 1); 2 the row's env index is
                                outside the handle (compared before it is used as an address); 3 the row's parameters or either
                                perturbed value are outside the parameter's limits (mass, kp scale > 0; friction, frictionloss >= 0;
                                all finite), or e is zero or not finite: nothing is stepped.  Nonzero: the column is zeros */
  uint32_t* contact_mask_fd; /* [n, npar, 2] the contact mask after the step of the + and of the - row (0 for a column that did not
                                step); the trailing kinematics + collision pass is skipped when this is NULL */
} KParamFdDev;
/* PER COLUMN: e as above, plus = fl(p_k + e), minus = fl(p_k - e); the two rows run kmanip_rollout's sub-step loop for one step (nsub
 * == 0: the model's n_sub_steps; the handle's solver) from the row's state and warm start + warm_offset, with every constant derived
 * from the parameters exactly as kmanip_set_env_params derives it; entry (r, c, .) = [tangent_diff(qpos+, qpos-) ; qvel+ - qvel-] /
 * fl(2.0 * e), a division.  The derivative in the friction loss AT 0 is refused (status 3), not faked: its rows exist only above 0.
 * ONE launch on `stream`.  No allocation, no synchronisation, no host copy.  THE HANDLE IS READ ONLY, and the call works on a handle
 * that never had per-env parameters without changing which kernels its steps use.  n == 0 or wrt == 0 succeeds and does nothing.
 * ERRORS: a NULL handle, `in` or `out`, n < 0, nsub < 0, n > num_envs with a NULL env_index, wrt bits outside the KM_EP_N lowest, a
 * non-finite warm_offset, an eps[k] of a selected parameter that is not finite or not > 0, wrt != 0 with a NULL deriv_t, or
 * 2 * npar * n beyond int return nonzero with kmanip_last_error set, launch nothing and leave the outputs untouched.
 * OUT OF SCOPE: parameters outside KM_EP_*, analytic derivatives, more than one step. */
KMANIP_API int kmanip_param_fd(KHandle h, const KParamFdIn* in, int n, int nsub, const KParamFdDev* out, void* stream);

/* Per-env visual parameters (visual domain randomisation of the camera renders).  Storage is
 * double[KM_VP_N][num_envs], struct-of-arrays like KM_EP_*: element (k, env) at k * num_envs + env.
 *   index  name                  default        meaning
 *   0-2    KM_VP_CUBE_RGB        1 0 0          cube material colour
 *   3-5    KM_VP_TABLE_RGB       .2 .2 .2       table colour
 *   6-8    KM_VP_ROBOT_RGB       .647059 x 3    the visible finger spheres and the link capsules (kmanip_set_render_links)
 *   9-11   KM_VP_BACKGROUND_RGB  0 0 0          pixels whose ray hits nothing
 *   12     KM_VP_AMBIENT         0.4            headlight ambient
 *   13     KM_VP_HEADLIGHT       0.4            headlight diffuse
 *   14     KM_VP_DIRECTIONAL     1.0            scale on the three 0.3 directional lights
 *   15-17  KM_VP_CAM_OFFSET      0 0 0          metres, added to cam_pos[c] of every camera, in cam_link's frame (world for
 *                                               top / head); the camera keeps tracking its target body
 * Object pixel of material m: round_half_up(255 I rgb_m[ch]) with
 *   I = min(1, ambient + headlight max(0, -n.d) + directional sum_l 0.3 max(0, n.L_l))  (d the unit ray direction);
 * background pixel: round_half_up(255 bg[ch]).  Env e with offset o renders what a model whose cam_pos is shifted by o renders
 * (gym_kmanip_amd/model.py with_visual_params); depth images use the offset and ignore colours and lights.  Physics, observations,
 * rewards and done bytes never depend on these values.  Limits: colours in [0, 1], light terms finite and >= 0, |offset
 * component| <= 0.25 m. */
enum {
  KM_VP_CUBE_RGB = 0, KM_VP_TABLE_RGB = 3, KM_VP_ROBOT_RGB = 6, KM_VP_BACKGROUND_RGB = 9, KM_VP_AMBIENT = 12, KM_VP_HEADLIGHT = 13,
  KM_VP_DIRECTIONAL = 14, KM_VP_CAM_OFFSET = 15, KM_VP_N = 18
};
/* Explicit values: params_dev DEVICE double[KM_VP_N][num_envs], read once `stream` has produced it; switches ranges mode off.
 * Validated on the device (one flag read back per call); a bad value returns nonzero and leaves the handle unchanged.
 * Synchronous (the whole device is idle when it returns).  The values are read when a render LAUNCHES: a render behind the steps
 * (kmanip_snapshot_render_state) uses the values in force at its launch.  params_dev == NULL returns to the default kernels,
 * bit-identical to a handle that never had visual parameters. */
KMANIP_API int kmanip_set_visual_params(KHandle h, const double* params_dev, void* stream);
/* The values in force into DEVICE double[KM_VP_N][num_envs] on `stream`: the defaults above when none are set; in ranges mode
 * the draw of every env's current episode. */
KMANIP_API int kmanip_get_visual_params(KHandle h, double* params_dev, void* stream);
/* Ranges mode: lo / hi HOST double[KM_VP_N].  Value k of env e in episode p is lo[k] + (hi[k] - lo[k]) * u_k (product rounded
 * before the sum), u_k a 53-bit uniform from Philox4x32-10 keyed by the seed with counter (global env id lo, hi, p,
 * KM_VP_CTR3 + k / 2): words (0, 1) of the block for even k, (2, 3) for odd k.  The renders evaluate the draw from the episode
 * counter, so every reset redraws and kmanip_set_seed / kmanip_set_episode move the draw as they move the cube spawn; in ranges
 * mode kmanip_snapshot_render_state copies the episode counters with qpos, and a render of that snapshot draws from the copy.
 * lo > hi or a value outside the limits above is refused (handle unchanged).  NULL, NULL turns ranges mode off and keeps the
 * values of every env's current episode as explicit values.  Synchronous. */
#define KM_VP_CTR3 0x100u
KMANIP_API int kmanip_set_visual_param_ranges(KHandle h, const double* lo, const double* hi);

KMANIP_API int kmanip_num_envs(KHandle h);
KMANIP_API const char* kmanip_last_error(KHandle h);   /* h may be NULL: error of the last failed create */
KMANIP_API const char* kmanip_version(void);

/* Replaces KManipEnvSim.k_close (env_sim.py:202-203). */
KMANIP_API void kmanip_destroy(KHandle h);

#ifdef __cplusplus
}
#endif
#endif /* KMANIP_H */
