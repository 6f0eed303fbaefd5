"""Where the MFMA waves of the 160-row 12-wave GEMM forms (csrc/gemm_lc.hip: gemm_lc3_kernel, gemm_lc3g_kernel) spend their time: a
-DLC_STAMPS build (make -C clip-based-cross-modal-hashing_amd/csrc BUILD=build_st EXTRA=-DLC_STAMPS; CMH_LIB=.../build_st/libcmh.so).
Per workgroup, MFMA wave 0, shader-clock ticks: the kernel | until the first stage has landed | inside the K loops | from a K loop's
end to the end of its epilogue | from there to the next tile's first K-step (tile set-up; the first tile's: the fragment preload);
and the 100 MHz wall clock over the kernel: clock = ticks / wall.  A stamp reads the clock through the scalar memory path and waits for
it, so the next stage's first fragments have landed by then as well: the tile switch reads a little high.
    python3 tools/lc3_stamps.py            every shape under CMH_LC3_DGE=0 (gemm_lc3_kernel) and unset (gemm_lc3g_kernel takes c_fc)"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cmh_native as N  # noqa: E402

dev = torch.device("cuda:0")
EPI_QKV = N.EPI_BIAS | N.EPI_OUT_BF16
EPI_FC1 = EPI_QKV | N.EPI_QUICKGELU
SHAPES = {"v_qkv": (12800, 2304, 768, EPI_QKV), "v_fc1": (12800, 3072, 768, EPI_FC1), "t_fc1": (10499, 2048, 512, EPI_FC1),
          "v_fc1_nostore": (12800, 3072, 768, EPI_FC1 | 256)}
N.set_gemm_lc(9)
for name, (M, Nn, K, epi) in SHAPES.items():
    x = torch.randn(M, K, device=dev).bfloat16()
    w = (torch.randn(Nn, K, device=dev) * K ** -0.5).bfloat16()
    b = torch.randn(Nn, device=dev)
    out = torch.empty(M, Nn, dtype=torch.bfloat16, device=dev)

    def launch():
        N.check(N.lib().cmh_linear_gemm(N.BF16, N.ptr(x), N.ptr(w), N.ptr(b), None, N.ptr(out), M, Nn, K, epi, N.stream_ptr(dev)), "gemm")
    for dge in ("0", None):
        if dge is None:
            os.environ.pop("CMH_LC3_DGE", None)
        else:
            os.environ["CMH_LC3_DGE"] = dge
        for _ in range(200):        # ~10 ms of back-to-back launches: the clock settles
            launch()
        torch.cuda.synchronize()
        N.prof_gemm_begin(64)
        for _ in range(40):
            launch()
        disp_us = N.prof_gemm_end()[0] * 1e3 / 40
        buf = np.zeros(256 * 8, dtype=np.uint64)
        assert N.lib().cmh_debug_lc_stamps(buf.ctypes.data_as(ctypes.c_void_p)) == 0
        s = buf.reshape(256, 8).astype(np.float64)[:min(256, -(-M // 160) * (Nn // 256))]
        s = s[s[:, 6] == s[:, 6].max()]          # the workgroups with the most tiles set the launch's length
        tot, wall, first, kl, ep, ks, tiles, gap = s.mean(0)
        ghz = tot / (wall * 10.0) if wall else 0.0
        form = "lc3 " if dge == "0" or not (epi & N.EPI_QUICKGELU) else "lc3g"
        print(f"{name:13s} {form}: {tiles:.0f} tiles, {ks:.0f} K-steps | kernel {tot:7.0f} ticks = {wall / 100:6.2f} us -> {ghz:4.2f} GHz "
              f"(dispatch {disp_us:6.2f} us) | first stage {first:5.0f} | K loops {kl:7.0f} = {kl / max(ks, 1):5.0f} per K-step "
              f"| epilogues {ep:6.0f} = {ep / max(tiles, 1):5.0f} per tile | tile set-up {gap:5.0f} = {gap / max(tiles, 1):4.0f} per tile "
              f"| K loop's end to the next K loop's start {(ep + gap) / max(tiles, 1):5.0f}", flush=True)
