"""Rate of the layered residual towers (csrc/nn_layered.hip), reported and not gated: stand-alone forward passes timed one by one with HIP
events — after 3 warm-up passes the median of 15 — for ResnetPV 6 x 192, 10 x 256, 20 x 256 and 6 x 512 on 15x15 and 10 x 256 on 20x20, batches
of 1024 and 4096 positions, on the whole chip and with a launch width of 64 compute units on a CU-masked stream.  At 6 x 128 the layered tower
(AGX_NN_LAYERED=1) next to the default kernel.  Every side is a child process of its own under its own `timeout`; the first one that fails ends
the run.  TFLOP/s count 2 x the multiply-adds of the convolutions per position (input 25 Cin F, a residual block 18 F^2, the policy head's 3x3
9 F^2, per cell) against 2 500 TFLOP/s dense fp16 MFMA for 256 compute units, scaled by the compute units in use: an end-to-end rate over
peak, not a kernel counter.  Launches per pass: 1 input + 2 per block + the policy conv + the heads + the value head (per slice of
plane_boards positions; one slice at these sizes).

A pass under a kernel trace (`rocprofv3 --kernel-trace -- python scripts/nn_layered_rate.py --trace-child ...`, a run of its own) gives
the share of a pass that is gaps between kernels: `--gaps <kernel trace csv>` prints it.

Usage: python scripts/nn_layered_rate.py [output json]        (writes profiles/nn_layered_rate.json by default)"""
import ctypes
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, PASSES = 3, 15
CHIP_PEAK_TFLOPS, CHIP_CUS = 2500.0, 256
CHILD_TIMEOUT = 240
WIDE = [(15, 15, 6, 192), (15, 15, 10, 256), (15, 15, 20, 256), (15, 15, 6, 512), (20, 20, 10, 256)]
BATCHES = [1024, 4096]
WIDTHS = [0, 64]                                                # 0: every compute unit


def flops_per_position(rows, cols, blocks, filters, in_channels=32):
    return 2.0 * rows * cols * (25 * in_channels * filters + blocks * 18 * filters * filters + 9 * filters * filters)


def launches_per_pass(blocks):
    return 1 + 2 * blocks + 1 + 1 + 1


def child(rows, cols, blocks, filters, trace_only=False):
    """one network in this process: every (batch, width) -> a JSON line on stdout"""
    from alphagomoku_amd import lib, check, selfplay, synthetic
    from alphagomoku_amd.networks import AGNetwork, DeviceBuffer
    cus = ctypes.c_int()
    check(lib.agx_device_cu_count(ctypes.byref(cus)))
    masked = selfplay.chip_slices(cus.value // 64)[0][0] if cus.value >= 128 else None   # a stream that owns 64 compute units
    desc = synthetic.net_desc(rows=rows, cols=cols, blocks=blocks, filters=filters)
    net = AGNetwork(desc)
    net.loadWeights(synthetic.make_weights(desc)[0])
    hw = rows * cols
    rows_out = []
    for boards in ([1024] if trace_only else BATCHES):
        f = synthetic.random_features(boards, rows, cols, seed=5)
        bufs = [DeviceBuffer(f.nbytes), DeviceBuffer(boards * hw * 4), DeviceBuffer(boards * 3 * 4)]
        bufs[0].upload(f)
        for width in ([0] if trace_only else WIDTHS):
            stream = masked if width else None
            check(lib.agx_net_set_launch_width(net._net, width))
            timer = ctypes.c_void_p()
            check(lib.agx_timer_create(ctypes.byref(timer)))
            times = []
            for i in range(WARMUP + PASSES):
                check(lib.agx_timer_start(timer, stream))
                net.forwardDevice(bufs[0].ptr, boards, bufs[1].ptr, bufs[2].ptr, stream)
                check(lib.agx_timer_stop(timer, stream))
                ms = ctypes.c_float()
                check(lib.agx_timer_elapsed_ms(timer, ctypes.byref(ms)))
                if i >= WARMUP:
                    times.append(ms.value)
            check(lib.agx_timer_destroy(timer))
            ms = statistics.median(times)
            in_use = width if width else cus.value
            tflops = flops_per_position(rows, cols, blocks, filters) * boards / ms * 1e-9
            layered = os.environ.get("AGX_NN_LAYERED", "") == "1" or filters > 128   # (the default kernels: the tower and the value head)
            rows_out.append(dict(board="%dx%d" % (rows, cols), network="%dx%d" % (blocks, filters), positions=boards, compute_units=in_use,
                                 layered=layered, ms=round(ms, 4), ms_min=round(min(times), 4),
                                 ms_max=round(max(times), 4), positions_per_s=round(boards / ms * 1e3), tflops=round(tflops, 1),
                                 of_mfma_peak=round(tflops / (CHIP_PEAK_TFLOPS * in_use / CHIP_CUS), 3), launches=launches_per_pass(blocks) if layered else 2))
        for b in bufs:
            b.free()
    net.close()
    for r in rows_out:
        print("RATE " + json.dumps(r), flush=True)


def gaps(path):
    """share of the traced window in which no kernel of the layered tower ran: 1 - sum of kernel durations / (last end - first start), over
    the kernels of the last half of the trace (the warm-up is in the first)"""
    with open(path) as f:
        spans = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    spans = spans[len(spans) // 2:]
    busy = sum(e - s for s, e, _ in spans)
    window = spans[-1][1] - spans[0][0]
    print(json.dumps(dict(kernels=len(spans), busy_ms=round(busy * 1e-6, 4), window_ms=round(window * 1e-6, 4), gap_share=round(1.0 - busy / window, 4))))


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--child", "--trace-child"):
        child(*(int(a) for a in sys.argv[2:6]), trace_only=sys.argv[1] == "--trace-child")
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--gaps":
        gaps(sys.argv[2])
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nn_layered_rate.json")
    sides = [(shape, None) for shape in WIDE] + [((15, 15, 6, 128), "0"), ((15, 15, 6, 128), "1")]
    results = []
    for shape, layered in sides:
        env = {k: v for k, v in os.environ.items() if k != "AGX_NN_LAYERED"}
        if layered is not None:
            env["AGX_NN_LAYERED"] = layered
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in shape]
        run = subprocess.run(cmd, capture_output=True, text=True, env=env)
        sys.stdout.write(run.stdout)
        if run.returncode != 0:                                 # nothing more is started on the device behind a side that failed
            sys.stderr.write(run.stderr[-4000:])
            sys.exit("side %s (AGX_NN_LAYERED=%s) ended with status %d" % (shape, layered, run.returncode))
        results += [json.loads(line[5:]) for line in run.stdout.splitlines() if line.startswith("RATE ")]
    narrow = {(r["positions"], r["compute_units"], r["layered"]): r for r in results if r["network"] == "6x128"}
    ratios = [dict(positions=p, compute_units=c, layered_over_default=round(narrow[(p, c, False)]["ms"] / narrow[(p, c, True)]["ms"], 3))
              for (p, c, lay) in sorted(narrow) if lay]
    with open(out, "w") as f:
        json.dump(dict(method="median of %d forward passes after %d warm-up passes, HIP events, one child process per network" % (PASSES, WARMUP),
                       peak="%.0f TFLOP/s dense fp16 for %d compute units, scaled to the compute units in use" % (CHIP_PEAK_TFLOPS, CHIP_CUS),
                       rates=results, narrow_6x128_layered_over_default=ratios), f, indent=1)
        f.write("\n")
    print("wrote %s" % out)


if __name__ == "__main__":
    main()
