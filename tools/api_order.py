"""One pass over the host API for comparing the HIP runtime calls of two library builds, in order: run it once per
build (GV_LIB_AB) under HIP API tracing and compare the ordered lists of API names, e.g.
  GV_QUEUE_PROBE=0 GV_LIB_AB=tools/_ab/parent.so rocprofv3 --hip-trace --output-format csv -d out -o parent -- python3 tools/api_order.py
GV_QUEUE_PROBE=0: the probe's round count depends on timing.  Every step is followed by a synchronize.
python3 tools/api_order.py planner  runs the planner calls instead: inflate, score_trajectories, nav_field, score_nav with
host and device poses and pinned and pageable destinations.
python3 tools/api_order.py compare a_hip_api_trace.csv b_hip_api_trace.csv [--no-alloc]  prints the first differences;
--no-alloc leaves hipMalloc and hipFree out of both lists (a change of who owns which buffer moves only those)."""
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


def names(path, no_alloc=False):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Function"] for r in rows if not (no_alloc and r["Function"] in ("hipMalloc", "hipFree"))]


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        no_alloc = "--no-alloc" in sys.argv[4:]
        a, b = names(sys.argv[2], no_alloc), names(sys.argv[3], no_alloc)
        diff = [(i, p, q) for i, (p, q) in enumerate(zip(a, b)) if p != q]
        print(f"{len(a)} and {len(b)} HIP API calls, {len(diff)} positions differ" + ("" if diff or len(a) != len(b) else ": identical order"))
        for i, p, q in diff[:20]:
            print(f"  #{i}: {p}  |  {q}")
    elif sys.argv[1:] == ["planner"]:
        run_planner()
    else:
        run()
