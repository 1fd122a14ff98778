#!/usr/bin/env python3
"""Per-kernel HIP-event times of one device-resident step for arbitrary sizes: profile_shape.py H W K [filters] [F]
Environment switches: EXACT=1 (exact_window plan), ONE_PASS=1 (never block-wise), DYN=0/1/2 (dynamic_tiles), FORMAT=1/2 (plan
option map_format: fp16 / bf16 result maps; 0 or unset: fp32), REGION=1..4 (plan option output_region), RECT=same | valid | off_h,off_w,out_h,out_w
(fftconv_plan_set_output_rect: the "same" / "valid" rectangle of the K x K kernels, or any rectangle of the window), RECT_STORE=0/1 (plan
option rect_store: 0 stages the window and crops the rectangle, the A/B partner of the output kernel's own rectangle store),
IMAGES=B (an image batch: set_images of B images per step; the figures are per step of B x filters maps), IMAGE_WALK=0/1 (plan option
image_walk: the spectral-row kernel walks over images), BATCH_MAPS=n, ROWS_GROUP=n (plan options batch_maps, rows_group)"""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, util
fc = util.load_package()
H, W, K = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
n = int(sys.argv[4]) if len(sys.argv) > 4 else 64
F = int(sys.argv[5]) if len(sys.argv) > 5 else 1
opts = {"exact_window": 1} if os.environ.get("EXACT") else None
if os.environ.get("ONE_PASS"): opts = dict(opts or {}, blockwise=1)      # never block-wise (A/B of the overlap-save blocks)
FORMAT = int(os.environ.get("FORMAT") or 0)      # element format of the maps (A/B of the 16-bit output path)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
B = int(os.environ.get("IMAGES") or 1)
img = torch.from_numpy(rng.random((B, F, W, H), dtype=np.float32)).to(dev)
ker = torch.from_numpy(rng.random((n, F, K, K), dtype=np.float32)).to(dev)
with fc.Plan(H, W, F, K, K, options=opts) as p:
    i = p.info
    if os.environ.get("DYN"): p.set_option("dynamic_tiles", int(os.environ["DYN"]))      # tile queue of the column kernels on / off (A/B)
    if FORMAT: p.set_option("map_format", FORMAT)
    region = ""
    if os.environ.get("REGION"):
        p.set_option("output_region", int(os.environ["REGION"])); region = " output_region %s" % os.environ["REGION"]
    if os.environ.get("RECT"):
        r = os.environ["RECT"]
        rect = ((K - 1) // 2, (K - 1) // 2, H, W) if r == "same" else (K - 1, K - 1, H - K + 1, W - K + 1) if r == "valid" else tuple(int(x) for x in r.split(","))
        if os.environ.get("RECT_STORE"): p.set_option("rect_store", int(os.environ["RECT_STORE"]))
        p.set_output_rect(*rect)
        region = " rectangle %s (rect_direct %d)" % (rect, p.get_option("rect_direct"))
    if os.environ.get("BATCH_MAPS"): p.set_option("batch_maps", int(os.environ["BATCH_MAPS"]))
    if os.environ.get("ROWS_GROUP"): p.set_option("rows_group", int(os.environ["ROWS_GROUP"]))
    if os.environ.get("IMAGE_WALK"):
        p.set_option("image_walk", int(os.environ["IMAGE_WALK"])); region += " image_walk %s (active %d)" % (os.environ["IMAGE_WALK"], p.get_option("image_walk_active"))
    if B > 1: region += " images %d" % B
    i = p.info
    out = torch.empty((B * n, i.out_w, i.out_h), dtype=torch.int16 if FORMAT else torch.float32, device=dev)
    def step():
        if B > 1: p.set_images_device(img.data_ptr(), B)
        else: p.set_image_device(img.data_ptr())
        p.convolve_packed_device(n, ker.data_ptr(), K, K, out.data_ptr())
    for _ in range(30): step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20): step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 20
    p.set_option("profile", 1); p.profile(reset=True)
    for _ in range(5): step()
    torch.cuda.synchronize()
    pr = p.profile(reset=True)
    print("%s maps " % ("fp32", "fp16", "bf16")[FORMAT] + "%dx%d K=%d F=%d n=%d window %dx%d%s transform %dx%d%s spec %d: %.1f us/step  %.1f Gpx/s | " % (H, W, K, F, n, i.fft_h, i.fft_w, region, i.transform_h, i.transform_w,
          (" x%d blocks" % p.get_option("blockwise")) if p.get_option("blockwise") else "", p.get_option("specialised_kernels"), dt * 1e6, B * n * i.fft_h * i.fft_w / dt / 1e9) +
          "  ".join("%s %.1f us x%d" % (k, v["ms"] / max(1, v["launches"]) * 1e3, v["launches"] // 5) for k, v in pr.items()))
