"""Rate of the run-time-shaped network kernel (csrc/nn_any_board.hip) next to the specialised 15x15 / 20x20 kernels, in one process on one GPU:
the method of tests/test_nn_gpu.py::test_network_rate_floor (4096 boards, 3 warm-up and 5 timed launches).  The lines go to
profiles/any_board_rate.txt.  Usage: python scripts/nn_any_board_rate.py [output file]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_nn_any_board_gpu import measure_tflops  # noqa: E402


def main():
    lines = []
    for rows, cols, blocks, filters in [(20, 20, 10, 128), (20, 20, 2, 64), (15, 15, 6, 128)]:
        os.environ["AGX_NN_ANY_BOARD"] = "0"
        special = measure_tflops(rows, cols, blocks, filters)
        os.environ["AGX_NN_ANY_BOARD"] = "1"
        general = measure_tflops(rows, cols, blocks, filters)
        lines.append("%dx%d %dx%d: specialised %.0f TFLOP/s, any-board %.0f TFLOP/s, ratio %.3f" % (rows, cols, blocks, filters, special, general, general / special))
    os.environ["AGX_NN_ANY_BOARD"] = "0"
    for rows, cols, blocks, filters in [(19, 19, 10, 128), (12, 12, 6, 128)]:
        lines.append("%dx%d %dx%d: any-board %.0f TFLOP/s" % (rows, cols, blocks, filters, measure_tflops(rows, cols, blocks, filters)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
