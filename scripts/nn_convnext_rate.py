"""Rate of the ConvNeXt tower (csrc/nn_convnext.hip), reported and not gated: stand-alone launches timed one by one with HIP events, 6 x 128 and
10 x 128 on 15x15 and 10 x 128 on 20x20 (ConvNextPVQMraw, all four heads), batches of 1 664 and 6 656 positions, on 64 compute units through
a CU-masked stream (launch width 64) and on the whole chip; after 3 warm-up launches the median of 21.  Next to every line the residual tower
(ResnetPVQ) of the same blocks x filters from the same process, for scale.  The lines go to profiles/nn_convnext_rate.txt.
Usage: python scripts/nn_convnext_rate.py [output file]"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphagomoku_amd import lib, check, selfplay, synthetic  # noqa: E402
from alphagomoku_amd.networks import AGNetwork, DeviceBuffer  # noqa: E402

WARMUP, LAUNCHES = 3, 21


def median_ms(net, moves_left, rows, cols, boards, stream, width):
    hw = rows * cols
    f = synthetic.random_features(boards, rows, cols, seed=5)
    bufs = [DeviceBuffer(f.nbytes), DeviceBuffer(boards * hw * 4), DeviceBuffer(boards * 3 * 4), DeviceBuffer(boards * hw * 2 * 4), DeviceBuffer(boards * hw * 4)]
    bufs[0].upload(f)
    check(lib.agx_net_set_launch_width(net._net, width))
    timer = ctypes.c_void_p()
    check(lib.agx_timer_create(ctypes.byref(timer)))
    times = []
    for i in range(WARMUP + LAUNCHES):
        check(lib.agx_timer_start(timer, stream))
        net.forwardDevice(bufs[0].ptr, boards, bufs[1].ptr, bufs[2].ptr, stream, bufs[3].ptr, bufs[4].ptr if moves_left else None)
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
    lines = ["network kernels, ms per launch (median of %d after %d warm-up launches) and positions/s; %d compute units" % (LAUNCHES, WARMUP, cus.value)]
    for rows, cols, blocks in [(15, 15, 6), (15, 15, 10), (20, 20, 10)]:
        cd = synthetic.convnext_desc(rows, cols, blocks, 128, 1)
        convnext = AGNetwork(cd)
        convnext.loadWeights(synthetic.make_convnext_weights(cd)[0])
        rd = synthetic.net_desc(rows=rows, cols=cols, blocks=blocks, filters=128, action_values=1)
        resnet = AGNetwork(rd)
        resnet.loadWeights(synthetic.make_weights(rd)[0])
        for boards in (1664, 6656):
            for where, stream, width in (("64 CUs", masked, 64), ("whole chip", None, 0)):
                a = median_ms(convnext, 1, rows, cols, boards, stream, width)
                b = median_ms(resnet, 0, rows, cols, boards, stream, width)
                lines.append("%dx%d %2dx128 %4d positions, %-10s: ConvNextPVQMraw %8.3f ms %10.0f positions/s | ResnetPVQ %8.3f ms %10.0f positions/s | x %.2f"
                             % (rows, cols, blocks, boards, where, a, boards / a * 1e3, b, boards / b * 1e3, b / a))
        convnext.close()
        resnet.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
