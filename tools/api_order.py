"""One pass over the host API for comparing the HIP runtime calls of two library builds, in order: run it once per
build (GV_LIB_AB) under HIP API tracing and compare the ordered lists of API names, e.g.
  GV_QUEUE_PROBE=0 GV_LIB_AB=tools/_ab/parent.so rocprofv3 --hip-trace --output-format csv -d out -o parent -- python3 tools/api_order.py
GV_QUEUE_PROBE=0: the probe's round count depends on timing.  Every step is followed by a synchronize.
python3 tools/api_order.py planner  runs the planner calls instead: inflate, score_trajectories, nav_field, score_nav with
host and device poses and pinned and pageable destinations.
python3 tools/api_order.py pose  runs the pose family on a fresh handle: kNN depth, poses of 1 and of 300 boxes (the second
regrows the result block), the ground plane with and without its mask, the ground-removed pose with and without boxes,
the vision post-process, a vision tick, a PCA tick with static and dynamic boxes, kNN depth again.
python3 tools/api_order.py shard  runs the sharded frame on a fresh handle with a one-rank communicator (it sets
GV_QUEUE_PROBE=0 itself): process_frame_sharded plain, with KEEP_COUNTS, and with everything it can keep plus boxes and
poses; six frames in flight; the stage timing; the three-rank emulation; comm_destroy and one plain frame.  RCCL's own HIP
calls are in both builds' traces alike.
python3 tools/api_order.py compare a_hip_api_trace.csv b_hip_api_trace.csv [--no-alloc] [--no-query]  prints the first
differences; --no-alloc leaves hipMalloc and hipFree out of both lists (a change of who owns which buffer moves only
those), --no-query hipStreamQuery (the result block's wait asks the stream once per 4096 spins: how often is timing)."""
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
    h.close()


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
