"""Rate of the bottleneck tower (the bottleneck block of csrc/nn_any_board.hip), reported and not gated: stand-alone launches timed one by one with HIP events, BottleneckPVQ
6 x 128 and 10 x 128 on 15x15 and 10 x 128 on 20x20, batches of 1 664 and 6 656 positions, on 64 compute units through a CU-masked stream
(launch width 64) and on the whole chip; after 3 warm-up launches the median of 21.  Next to every line the residual tower (ResnetPVQ) of the
same blocks x filters from the same process.  TFLOP/s count 2 x the multiply-adds of the convolutions per position (input 25 Cin F, a
bottleneck block 7.25 F^2, a residual block 18 F^2, the two 3x3 head convolutions 9 F^2 each, per cell) against 2 500 TFLOP/s dense fp16 MFMA
for the whole chip, scaled by the compute units in use.  The lines go to profiles/nn_bottleneck_rate.txt.
Usage: python scripts/nn_bottleneck_rate.py [output file]"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphagomoku_amd import lib, check, selfplay, synthetic  # noqa: E402
from alphagomoku_amd.networks import AGNetwork, DeviceBuffer  # noqa: E402

WARMUP, LAUNCHES = 3, 21
CHIP_PEAK_TFLOPS = 2500.0


def flops_per_position(desc, block_macs):
    f, hw = desc["filters"], desc["rows"] * desc["cols"]
    return 2.0 * hw * (25 * desc["in_channels"] * f + desc["blocks"] * block_macs * f * f + 2 * 9 * f * f)


def median_ms(net, rows, cols, boards, stream, width):
    hw = rows * cols
    f = synthetic.random_features(boards, rows, cols, seed=5)
    bufs = [DeviceBuffer(f.nbytes), DeviceBuffer(boards * hw * 4), DeviceBuffer(boards * 3 * 4), DeviceBuffer(boards * hw * 2 * 4)]
    bufs[0].upload(f)
    check(lib.agx_net_set_launch_width(net._net, width))
    timer = ctypes.c_void_p()
    check(lib.agx_timer_create(ctypes.byref(timer)))
    times = []
    for i in range(WARMUP + LAUNCHES):
        check(lib.agx_timer_start(timer, stream))
        net.forwardDevice(bufs[0].ptr, boards, bufs[1].ptr, bufs[2].ptr, stream, bufs[3].ptr)
        check(lib.agx_timer_stop(timer, stream))
        ms = ctypes.c_float()
        check(lib.agx_timer_elapsed_ms(timer, ctypes.byref(ms)))
        if i >= WARMUP:
            times.append(ms.value)
    check(lib.agx_timer_destroy(timer))
    for b in bufs:
        b.free()
    return statistics.median(times)


def main():
    cus = ctypes.c_int()
    check(lib.agx_device_cu_count(ctypes.byref(cus)))
    slices = cus.value // 64
    masked = selfplay.chip_slices(slices)[0][0] if slices > 1 else None      # a stream that owns 64 compute units
    lines = ["network kernels, ms per launch (median of %d after %d warm-up launches), positions/s, TFLOP/s and fraction of the MFMA peak of the "
             "compute units in use; %d compute units" % (LAUNCHES, WARMUP, cus.value)]
    for rows, cols, blocks in [(15, 15, 6), (15, 15, 10), (20, 20, 10)]:
        bd = synthetic.bottleneck_desc(rows, cols, blocks, 128, action_values=1)
        bottleneck = AGNetwork(bd)
        bottleneck.loadWeights(synthetic.make_bottleneck_weights(bd)[0])
        rd = synthetic.net_desc(rows=rows, cols=cols, blocks=blocks, filters=128, action_values=1)
        resnet = AGNetwork(rd)
        resnet.loadWeights(synthetic.make_weights(rd)[0])
        for boards in (1664, 6656):
            for where, stream, width in (("64 CUs", masked, 64), ("whole chip", None, 0)):
                peak = CHIP_PEAK_TFLOPS * ((64.0 / cus.value) if width else 1.0)
                a = median_ms(bottleneck, rows, cols, boards, stream, width)
                b = median_ms(resnet, rows, cols, boards, stream, width)
                ta = flops_per_position(bd, 7.25) * boards / a * 1e-9
                tb = flops_per_position(rd, 18.0) * boards / b * 1e-9
                lines.append("%dx%d %2dx128 %4d positions, %-10s: BottleneckPVQ %8.3f ms %10.0f positions/s %6.1f TFLOP/s %.2f of peak | "
                             "ResnetPVQ %8.3f ms %10.0f positions/s %6.1f TFLOP/s %.2f of peak | x %.2f"
                             % (rows, cols, blocks, boards, where, a, boards / a * 1e3, ta, ta / peak, b, boards / b * 1e3, tb, tb / peak, b / a))
        bottleneck.close()
        resnet.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
