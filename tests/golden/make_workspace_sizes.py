"""Record what every public workspace sizing function returns over a grid of shapes -> tests/golden/workspace_sizes.json.

Run it on the commit whose sizes are the contract (python tests/golden/make_workspace_sizes.py); tests/test_workspace_cpu.py holds
every later build to the file, value for value.  No device is needed, and none should be visible: sela_hip_encode_workspace_bytes
asks the current device for its CU count from 2048 frames on (encode_split_frames), so those rows go into "encode_device_dependent"
and are compared only where no device is visible.  GRID is imported by the tests: one list of shapes for the sizes and the carve.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FRAMES = (0, 1, 2, 63, 64, 65, 4096, 4097, 16384)  # 4096: the sample-tile edge
CHANNELS = (1, 2, 3, 8, 9, 255)                     # 8 / 9: the wide-decoder and interleave edge
STRIDES = (1, 2047, 2048, 2049, 4095, 65535)        # stride, or samples per channel
WINDOWS = (0, 1, 256)
WINDOW_SAMPLES = (1, 2049, 2050, 1 << 24)
PAYLOADS = (0, 4, 65536, 1001)                      # 1001: no multiple of 4
WHOLE_SAMPLES = (0, 1, 2047, 2048, 4095, 4096, 10 ** 7)

FRAMES_SHAPES = [(f, c, s) for f in FRAMES for c in CHANNELS for s in STRIDES]
# every argument combination that has to give SIZE_MAX, and its neighbour that does not
BY_TABLE_REFUSED = [(1 << 20, 1 << 20, 1 << 20), (1 << 20, 1 << 20, (1 << 20) - 1), (1 << 24, 128, 1), (1 << 24, 127, 1), (1 << 23, 255, 1)]
ENCODE_N_REFUSED = [(1, 0, 100), (1, 256, 100), (1, 2, 0), (1, 2, 65536), (1 << 24, 128, 1), (1 << 24, 127, 1), (1 << 23, 255, 65535), (1 << 30, 2, 1), (1 << 30, 3, 1),
                    (1 << 30, 4, 1)]
WHOLE_REFUSED = [(2048, 0), (2048, 256), (2048 << 31, 1), ((2048 << 31) - 1, 1), (2048 * 715827883, 2), (2048 * 715827882, 2), (2048 << 23, 255), (2048 << 24, 128)]

GRID = {
    "sela_hip_encode_workspace_bytes": [(f, c) for f in FRAMES if f < 2048 for c in CHANNELS],
    "encode_device_dependent": [(f, c) for f in FRAMES if f >= 2048 for c in CHANNELS],  # (sela_hip_encode_workspace_bytes)
    "sela_hip_decode_workspace_bytes": [(f, c) for f in FRAMES for c in CHANNELS],
    "sela_hip_index_workspace_bytes": [(p, m) for p in PAYLOADS + (1 << 32, (1 << 34) - 4) for m in (0, 4096)],
    "sela_hip_decode_i32_workspace_bytes": FRAMES_SHAPES + BY_TABLE_REFUSED,
    "sela_hip_decode_n_workspace_bytes": FRAMES_SHAPES + BY_TABLE_REFUSED,
    "sela_hip_verify_workspace_bytes": FRAMES_SHAPES + BY_TABLE_REFUSED,
    "sela_hip_verify_i32_workspace_bytes": FRAMES_SHAPES + BY_TABLE_REFUSED,
    "sela_hip_encode_i32_workspace_bytes": FRAMES_SHAPES + ENCODE_N_REFUSED,
    "sela_hip_encode_paired_workspace_bytes": FRAMES_SHAPES + ENCODE_N_REFUSED,
    "sela_hip_decode_windows_workspace_bytes": [(w, s, c) for w in WINDOWS for s in WINDOW_SAMPLES for c in CHANNELS],
    "sela_hip_decode_windows_whole_workspace_bytes": [(w, s, c) for w in WINDOWS for s in WINDOW_SAMPLES for c in CHANNELS],
    "sela_hip_encode_whole_workspace_bytes": [(n, c) for n in WHOLE_SAMPLES for c in CHANNELS] + WHOLE_REFUSED,
}
SIZE_MAX = (1 << 64) - 1


def function_of(key):
    return "sela_hip_encode_workspace_bytes" if key == "encode_device_dependent" else key


def measure(lib, key, args):
    return int(getattr(lib, function_of(key))(*args))


def main():
    from sela_amd import capi

    lib = capi.lib()
    assert lib.sela_hip_device_count() <= 0, "record the sizes where no device is visible"
    out = {key: [list(args) + [measure(lib, key, args)] for args in shapes] for key, shapes in GRID.items()}
    refused = sum(1 for rows in out.values() for row in rows if row[-1] == SIZE_MAX)
    path = os.path.join(HERE, "workspace_sizes.json")
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + "\n}\n")
    print(f"{path}: {sum(len(v) for v in out.values())} sizes, {refused} of them SIZE_MAX, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
