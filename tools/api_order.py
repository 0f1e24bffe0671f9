"""One pass over the host API for comparing the HIP runtime calls of two library builds, in order: run it once per
build (GV_LIB_AB) under HIP API tracing and compare the ordered lists of API names, e.g.
  GV_QUEUE_PROBE=0 GV_LIB_AB=tools/_ab/parent.so rocprofv3 --hip-trace --output-format csv -d out -o parent -- python3 tools/api_order.py
GV_QUEUE_PROBE=0: the probe's round count depends on timing.  Every step is followed by a synchronize.
python3 tools/api_order.py planner  runs the planner calls instead: inflate, score_trajectories, nav_field, score_nav with
host and device poses and pinned and pageable destinations; then the controller calls over them (run_controller): rollouts
from host and device controls, control steps into pinned and pageable memory with and without totals, the MPPI calls
without and with limits and a control cost, the dyn configuration and object set twice with score_dynamic from both pose
sources into both kinds of destination, three set_tracks, track updates from the host and fed with a control step behind
them, and a second set_inflation and inflate.
python3 tools/api_order.py pose  runs the pose family on a fresh handle: kNN depth, poses of 1 and of 300 boxes (the second
regrows the result block), the ground plane with and without its mask, the ground-removed pose with and without boxes,
the vision post-process, a vision tick, a PCA tick with static and dynamic boxes, kNN depth again.
python3 tools/api_order.py shard  runs the sharded frame on a fresh handle with a one-rank communicator (it sets
GV_QUEUE_PROBE=0 itself): process_frame_sharded plain, with KEEP_COUNTS, and with everything it can keep plus boxes and
poses; six frames in flight; the stage timing; the three-rank emulation; comm_destroy and one plain frame.  RCCL's own HIP
calls are in both builds' traces alike.
python3 tools/api_order.py compare a_hip_api_trace.csv b_hip_api_trace.csv [--no-alloc] [--no-query] [--no-register]  prints
the first differences; --no-alloc leaves hipMalloc and hipFree out of both lists (a change of who owns which buffer moves
only those), --no-query hipStreamQuery (the result block's wait asks the stream once per 4096 spins: how often is timing),
--no-register the __hipRegister* calls of the library's load (a build with one kernel more registers one function more)."""
import csv, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
    import gvamd
    from gvamd import synth
    g = synth.CONFIGS[1]["grid"]
    tfs = synth.transforms(True)
    x, y, z, _ = synth.cloud_uniform(1)
    bb, pp = synth.detections(3, 8), synth.lshape_poses(1, 8)
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution)
    h.synchronize()
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    h.synchronize()
    h.upload_xyz(x, y, z)
    h.synchronize()
    h.set_detections(gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST | gvamd.FRAME_KEEP_CELL_IDX, bboxes=bb, poses=pp)
    h.synchronize()
    for _ in range(8):
        h.enqueue_frame()
    h.synchronize()
    h.tick(bb, k_near=4, lidar_bin=True, lidar_raymarch=True)
    h.synchronize()
    h.set_inflation(0.3, 1.0)
    h.inflate()
    h.synchronize()
    for get in (h.hits, h.miss, h.cell_idx, h.bbox_id, h.ray_stats, h.costmap, h.log_odds):
        get()
        h.synchronize()
    h.close()


def run_planner():
    sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import gvamd
    import planner_time_common as common
    from gvamd import synth
    hip = common.load_hip()
    h = gvamd.GridVisionHIP(50, 20, 0.1)
    for t in range(4):
        h.update_map_poses(common.fill_poses(synth, h, 0.1, 40, 100 + t))
    h.set_inflation(0.35, 0.55, 10.0, 65)
    h.inflate()
    h.synchronize()
    h.set_footprint(((3.4, 1.0), (-1.1, 1.0), (-1.1, -1.0), (3.4, -1.0)))
    h.set_nav_config(253, 3)
    h.nav_field(np.array([[h.pos_x, h.pos_y], [h.pos_x + 3.0, h.pos_y - 2.0]], np.float32))
    h.synchronize()
    for K, P in ((7, 65), (40, 130), (2, 1)):     # the second batch makes every buffer grow
        poses = common.arcs(h, K, P, seed=K, start=(-4.0, 1.0))
        dptr = common.device_copy(hip, poses)
        pin_s, pin_p, pin_n = gvamd.PinnedI8(K * 16), gvamd.PinnedI8(K * P), gvamd.PinnedI8(K * 24)
        for dev in (None, dptr.value):
            src = None if dev else poses
            for pinned in (True, False):
                ts = pin_s.array.view(gvamd.TRAJ_SCORE_DTYPE) if pinned else np.zeros(K, gvamd.TRAJ_SCORE_DTYPE)
                tp = pin_p.array.view(np.uint8) if pinned else np.zeros(K * P, np.uint8)
                ns = pin_n.array.view(gvamd.NAV_SCORE_DTYPE) if pinned else np.zeros(K, gvamd.NAV_SCORE_DTYPE)
                h.score_trajectories_async(src, K, P, ts, tp, device_ptr=dev)
                h.score_nav_async(src, K, P, ns, device_ptr=dev)
                h.score_trajectories_async(src, K, P, ts, None, device_ptr=dev)
                h.synchronize()
            h.score_trajectories(poses, keep_pose_cost=True, device_ptr=dev)
            h.score_nav(poses, device_ptr=dev)
        h.inflate()
        h.synchronize()
        hip.hipFree(dptr)
        for p in (pin_s, pin_p, pin_n):
            p.close()
    run_controller(h, gvamd, np, common, hip)
    h.close()


def run_controller(h, gvamd, np, common, hip):
    """the controller calls over the layers run_planner made: every step followed by a synchronize"""
    synth = gvamd.synth
    steps = []
    step = steps.append
    K, P, dt = 40, 130, 0.1
    start = (h.pos_x - 4.0, h.pos_y + 1.0, 0.2)
    rng = np.random.default_rng(3)
    u = np.stack([rng.normal(1.0, 0.2, K * P), rng.normal(0.0, 0.2, K * P)], axis=1).astype(np.float32).reshape(K, P, 2)
    u_dev = common.device_copy(hip, u)
    nav_w, no_nav_w = gvamd.CriticWeights(1, 2, 4, 0, 1, 0), gvamd.CriticWeights(1, 2, 0, 0, 0, 0)
    pin_r, pin_t, pin_n, pin_d, pin_c = (gvamd.PinnedI8(16), gvamd.PinnedI8(K * 8), gvamd.PinnedF32(P * 2), gvamd.PinnedI8(K * 24),
                                        gvamd.PinnedI8(K * P))
    res_pin, tot_pin = pin_r.array.view(gvamd.CONTROL_RESULT_DTYPE), pin_t.array.view(np.uint64)
    res_pg, tot_pg, nom_pg = np.zeros(1, gvamd.CONTROL_RESULT_DTYPE), np.zeros(K, np.uint64), np.zeros(P * 2, np.float32)

    def control_steps(w=nav_w):
        for res, tot in ((res_pin, tot_pin), (res_pin, None), (res_pg, tot_pg), (res_pg, None)):
            step(lambda res=res, tot=tot: h.control_step_async(w, res, tot))

    step(lambda: h.set_motion_model(gvamd.MotionModel(gvamd.MOTION_DIFF, dt, 0)))
    step(lambda: h.rollout_async(start, u))
    step(lambda: h.rollout_async(start, u[:7, 0], constant=True, P=65))
    step(lambda: h.rollout_async(start, u.shape, device_ptr=u_dev.value))
    control_steps()
    control_steps(no_nav_w)
    # MPPI without limits, then with limits and gamma > 0
    step(lambda: h.set_mppi(gvamd.MppiConfig.of((0.3, 0.4), (-0.5, -1.5), (3.0, 1.5), 30.0)))
    for limits in (None, gvamd.MppiLimits.of(rate_up=(2.0, 3.0), rate_down=(3.0, 3.0), u_prev=(1.0, 0.0), min_turn_radius=1.5, gamma=0.05)):
        step(lambda limits=limits: h.set_mppi_limits(limits))
        step(lambda: h.mppi_set_nominal(u[0]))
        step(lambda: h.mppi_sample(K, 11, 0, wait=False))
        step(lambda: h.rollout_async(start, (K, P, 2), device_ptr=h.device_controls()[0]))
        step(lambda: h.mppi_update_async(nav_w, res_pin, tot_pin, pin_n.array))
        step(lambda: h.mppi_update_async(nav_w, res_pg, tot_pg, nom_pg))
        step(lambda: h.mppi_update_async(no_nav_w, res_pg))
        step(lambda: h.mppi_cycle_async(start, K, 11, 1, nav_w, res_pin, tot_pin, pin_n.array, shift=True))
        step(lambda: h.mppi_cycle_async(start, 7, 11, 2, nav_w, res_pg))
    # X13: each setter twice, the sampler with both pose sources and both destinations, then as a third critic
    cfgs = [gvamd.DynConfig.of(off_x=(-1.0, 0.5, 2.0), radius=1.1, influence_radius=r, cost_scaling_factor=2.0, quantum=0.05, t0=dt, dt=dt,
                               collision_cost=253, w_sum=1, w_max=2) for r in (3.0, 2.5)]
    sets = [gvamd.moving_objects(np.array([[h.pos_x + 2.0 * j, h.pos_y + 1.0, 0.3, 4.0, 2.0, 1.0, -0.5] for j in range(n)])) for n in (3, 2)]
    poses = common.arcs(h, K, P, seed=5, start=(-4.0, 1.0))
    poses_dev = common.device_copy(hip, poses)
    ds_pin, pc_pin = pin_d.array.view(gvamd.DYN_SCORE_DTYPE), pin_c.array.view(np.uint8)
    ds_pg, pc_pg = np.zeros(K, gvamd.DYN_SCORE_DTYPE), np.zeros(K * P, np.uint8)
    for cfg, objs in zip(cfgs, sets):
        step(lambda cfg=cfg: h.set_dyn_config(cfg))
        step(lambda objs=objs: h.set_moving_objects(objs))
        for src, dev in ((poses, None), (None, poses_dev.value)):
            step(lambda src=src, dev=dev: h.score_dynamic_async(src, K, P, ds_pin, pc_pin, device_ptr=dev))
            step(lambda src=src, dev=dev: h.score_dynamic_async(src, K, P, ds_pg, pc_pg, device_ptr=dev))
            step(lambda src=src, dev=dev: h.score_dynamic_async(src, K, P, ds_pg, None, device_ptr=dev))
        control_steps()
    # X14: three set_tracks (the third reuses a staging slot), updates from the host and fed, a control step behind them
    xy = np.array([[h.pos_x + 3.0 * j, h.pos_y - 1.0] for j in range(3)])
    dets = np.zeros(3, synth.LSHAPE_DTYPE)
    dets["px"], dets["py"], dets["qw"], dets["length"], dets["width"], dets["height"] = xy[:, 0] + 0.1, xy[:, 1], 1.0, 4.5, 2.0, 1.5
    tracks = np.zeros(3, gvamd.TRACK_DTYPE)
    tracks["slot"], tracks["id"], tracks["hits"], tracks["det"] = np.arange(3), 1 + np.arange(3), 5, -1
    tracks["x"], tracks["y"], tracks["qw"], tracks["length"], tracks["width"] = xy[:, 0], xy[:, 1], 1.0, 4.5, 2.0
    tracks["p00"], tracks["p01"], tracks["p11"] = 0.05, 0.02, 0.5
    dets_dev = common.device_copy(hip, dets)
    info_pg, out_pg = np.zeros(1, gvamd.TRACK_INFO_DTYPE), np.zeros(gvamd.TRACK_SLOTS, gvamd.TRACK_DTYPE)
    step(lambda: h.set_track_config(gvamd.TrackConfig.of(gate=2.0)))
    for n in (3, 2, 1):
        step(lambda n=n: h.set_tracks(tracks[:n], 10))
    step(lambda: h.track_update_async(dets, 0.05, info=info_pg, tracks=out_pg))
    step(lambda: h.track_update_async(dets, 0.05, feed=True))
    step(lambda: h.track_update_async(None, 0.05, feed=True, device_ptr=dets_dev.value, n=3))
    control_steps()
    step(lambda: h.score_dynamic_async(poses, K, P, ds_pg, None))
    step(h.get_tracks)
    step(lambda: h.set_inflation(0.3, 0.6, 8.0, 65))
    step(h.inflate)
    for s in steps:
        s()
        h.synchronize()
    for d in (u_dev, poses_dev, dets_dev):
        hip.hipFree(d)
    for p in (pin_r, pin_t, pin_n, pin_d, pin_c):
        p.close()


def run_pose():
    sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
    import ctypes as C
    import gvamd
    from gvamd import synth
    g = synth.CONFIGS[1]["grid"]
    tfs = synth.transforms(True)
    x, y, z, _ = synth.cloud_uniform(1)
    bb, many = synth.detections(1, 12), synth.detections(1, 300)
    st, dy = gvamd.filter_bboxes(bb)
    assert len(st) and len(dy)
    net = synth.network_outputs(len(dy))
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    steps = [lambda: h.upload_xyz(x, y, z),
             lambda: h.compute_depth_for_bboxes(st, 4),
             lambda: h.compute_bbox_pose(bb[:1]),
             lambda: h.compute_bbox_pose(many),
             lambda: h.segment_ground_plane(),
             lambda: h._ck(h._lib.gv_segment_ground_plane(h._h, C.c_double(0.04), C.c_int32(50), C.c_uint64(12345), None, None, None),
                           "segment_ground_plane"),
             lambda: h.compute_bbox_pose_ground_removed(bb),
             lambda: h.compute_bbox_pose_ground_removed(bb[:0]),
             lambda: h.vision_post_process(*net, dy),
             lambda: h.tick(bb, k_near=4, vision=True, net=net),
             lambda: h.tick(bb, k_near=4),
             lambda: h.compute_depth_for_bboxes(st, 4)]
    for step in steps:
        h.synchronize()
        step()
    h.synchronize()
    h.close()


def run_shard():
    os.environ["GV_QUEUE_PROBE"] = "0"
    sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
    import gvamd
    from gvamd import synth
    g = synth.CONFIGS[1]["grid"]
    tfs = synth.transforms(True)
    x, y, z, _ = synth.cloud_uniform(1)
    bb, pp = synth.detections(3, 8), synth.lshape_poses(1, 8)
    rm = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    keep_all = rm | gvamd.FRAME_KEEP_COUNTS | gvamd.FRAME_KEEP_CELL_IDX | gvamd.FRAME_BBOX_TEST
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])

    def six_in_flight():
        for _ in range(6):
            h.enqueue_frame_sharded()

    steps = [lambda: h.upload_xyz(x, y, z),
             lambda: h.comm_init(gvamd.GridVisionHIP.comm_unique_id(), 0, 1),
             lambda: h.process_frame_sharded(rm),
             lambda: h.process_frame_sharded(rm | gvamd.FRAME_KEEP_COUNTS),
             lambda: h.process_frame_sharded(keep_all, bboxes=bb, poses=pp),
             six_in_flight,
             lambda: h.time_frame_sharded_stages(2),
             lambda: h.frame_sharded_emulated(3, keep_all, bboxes=bb, poses=pp),
             h.comm_destroy,
             lambda: h.process_frame(keep_all, bboxes=bb, poses=pp)]
    for step in steps:
        h.synchronize()
        step()
    h.synchronize()
    h.close()


def names(path, skip=()):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Function"] for r in rows if r["Function"] not in skip]


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        skip = ("hipMalloc", "hipFree") * ("--no-alloc" in sys.argv[4:]) + ("hipStreamQuery",) * ("--no-query" in sys.argv[4:])
        a, b = names(sys.argv[2], skip), names(sys.argv[3], skip)
        if "--no-register" in sys.argv[4:]:
            a, b = ([n for n in l if not n.startswith("__hipRegister")] for l in (a, b))
        diff = [(i, p, q) for i, (p, q) in enumerate(zip(a, b)) if p != q]
        print(f"{len(a)} and {len(b)} HIP API calls, {len(diff)} positions differ" + ("" if diff or len(a) != len(b) else ": identical order"))
        for i, p, q in diff[:20]:
            print(f"  #{i}: {p}  |  {q}")
    elif sys.argv[1:] == ["planner"]:
        run_planner()
    elif sys.argv[1:] == ["pose"]:
        run_pose()
    elif sys.argv[1:] == ["shard"]:
        run_shard()
    else:
        run()
