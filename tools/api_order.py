"""One pass over the host API for comparing the HIP runtime calls of two library builds, in order: run it once per
build (GV_LIB_AB) under HIP API tracing and compare the ordered lists of API names, e.g.
  GV_QUEUE_PROBE=0 GV_LIB_AB=tools/_ab/parent.so rocprofv3 --hip-trace --output-format csv -d out -o parent -- python3 tools/api_order.py
GV_QUEUE_PROBE=0: the probe's round count depends on timing.  Every step is followed by a synchronize.
python3 tools/api_order.py compare a_hip_api_trace.csv b_hip_api_trace.csv  prints the first differences."""
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


def names(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Function"] for r in rows]


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        a, b = names(sys.argv[2]), names(sys.argv[3])
        diff = [(i, p, q) for i, (p, q) in enumerate(zip(a, b)) if p != q]
        print(f"{len(a)} and {len(b)} HIP API calls, {len(diff)} positions differ" + ("" if diff or len(a) != len(b) else ": identical order"))
        for i, p, q in diff[:20]:
            print(f"  #{i}: {p}  |  {q}")
    else:
        run()
