#!/usr/bin/env python3
"""bench.py -- SELA frame encode+decode throughput on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

(`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the second form itself and
prints the same ONE JSON line last on stdout.)

One "step" = one pass of the hot path over synthetic PCM that is already resident in HBM: encode to the
.sela frame stream, decode the stream back to PCM.  The HEADLINE (`value`) is the same job at every N, so that
lines of different N divide into an efficiency:

  track (default)   BASELINE.json configs[1], WEAK scaling: every rank encodes and decodes one 3-minute 16-bit
                    stereo 44.1 kHz track = 3875 frames of 2048 samples (rank r: album track 3 r, the album's
                    44.1 kHz tracks; N = 1: track 0).  For N > 1 the ranks all-gather the compressed frame sizes
                    over RCCL every step -- the only exchange the path has -- inside the timed
                    region.  value = N x 3875 x 2048 samples / step time.

Two more workloads ride along as extra blocks of the same line (and can be made the headline with --workload):

  album             BASELINE.json configs[3], STRONG scaling: the 100-track album (34/33/33 tracks at 44.1/48/96
                    kHz, 549,365 frames); the (track, frame) space is cut into N contiguous balanced ranges
                    (sela_amd.sharding.partition -- the reference's static partition, src/sela/encoder.cpp:58-73),
                    every rank encodes and decodes its range in batches of <= 65,536 frames, one all-gather of
                    the sizes per step; the gathered layout is checked against the reference's digest.  The
                    `album` block of the --gpus 1 line is the one-GPU anchor of the N > 1 lines' `album` blocks.
  decode10k         BASELINE.json configs[4], STRONG scaling, decode only: 10,000 frames encoded OUTSIDE the
                    timed region, every rank decodes its contiguous 1/N; no collective (output offsets are
                    frame x 2048 x channels x 2).

After W untimed warm-up steps (and, for W > 0, more until 0.2 s of them have run right before the timed
region, while the clocks settle), exactly K steps are timed back to back, bracketed by barrier +
torch.cuda.synchronize(), MAX over ranks: `ms_per_step` is that time / K and `value` follows from it.  (The
one-lane leg of the `lanes` block times K more steps of its own; the extra blocks time theirs.)

--dump-outputs DIR writes what the headline's last timed step computed -- the arrays a caller of the path
receives -- as DIR/<name>.npy (float32 / float64, under 64 MB in all): every frame offset of the rank's
stream, and the frame bytes and decoded PCM of a fixed, seeded sample of its frames.  The inputs are
synthetic and seeded, so two builds run with the same arguments can be compared output for output.

WHAT IS TIMED IS WHAT IS CHECKED: the timed steps run as two independent encode->decode chains in flight on two
HIP streams (`lanes`).  Every timed call leaves its status words in a slot of its own, all of them are OR-ed
after the timed region; the outputs each lane's LAST timed step left in its buffers (frame bytes, offsets, decoded
PCM) are compared on the device with those of a serial, synchronised step, and that step's with the CPU reference
(`timed_outputs`).

Rank 0 prints ONE JSON line: metric/value as BASELINE.json names them (Msamples/s, a sample = one stereo pair
that went through encode AND decode), plus
  "roofline"      the dominant kernel (k_encode_blocks): algorithmic bytes per launch / its average duration
                  measured with HIP events on the launch stream, against the 8 TB/s HBM peak; the resource that
                  actually binds the kernel (vector-ALU issue) is beside it as "binding"
  "cpu_baseline"  the reference (oracle/_ref, kind "reference") or the CPU restatement (kind "port") timed on
                  this box's host cores (rank 0) on a bounded sample of the same workload
  "e2e"           host-pointer API (H2D + kernels + D2H, steady_clock) and "file_to_file" (file read .. file
                  write, the reference's `sela -e` / `-d`), measured by host/sela_filebench (N = 1 only).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_CLOCK_GHZ = 2.4   # the ONE clock every issue-rate figure here and in DESIGN.md is priced against (MI355X peak engine clock)
VALU_ISSUE_PEAK_GIPS = 256 * 4 * PEAK_CLOCK_GHZ / 4  # wave-instructions/ns: 1024 SIMDs, one wave64 instruction per 4 cycles each
FP64_UNFUSED_PEAK_TOPS = 256 * 4 * 16 * PEAK_CLOCK_GHZ / 1e3  # vector FP64, one operation per lane and cycle: 39.3 (78.6 TFLOP/s counts an FMA as 2)
# unfused FP64 operations the reference's analysis needs per 2048-sample block:
# 101 lags x (2048 - lag) x (mul + add) for the autocorrelation + 4950 Schur column updates x 4
FP64_OPS_PER_BLOCK = 2 * sum(2048 - i for i in range(101)) + 4 * 4950
TRACK_SECONDS, SAMPLE_RATE, CHANNELS = 180, 44100, 2
ALBUM_BATCH_FRAMES = 65536
DECODE_RESIDENT_WAVES = 7 * 1024  # k_decode_frames: seven waves per SIMD (72 VGPRs, 5.7 KB of LDS per subframe)
DECODE10K_FRAMES, DECODE10K_TRACK = 10000, 2
ENCODE_TARGET_MSPS = 1000.0  # BASELINE.json north_star: >= 1 G stereo samples/s encode on one MI355X
METRIC = "Msamples/s encode+decode, 16-bit stereo 44.1kHz, 1/2/4/8 GPU; bit-exact vs CPU"  # BASELINE.json "metric"
WARMUP_SETTLE_S, SETTLE_BLOCK_S = 0.2, 0.05  # untimed steps right before a timed region (with --warmup W > 0), and their blocks
DUMP_FRAMES, DUMP_SEED = 1024, 20251015  # --dump-outputs: how many frames' bytes and PCM are written, and the seed that picks them
DUMP_BUDGET_BYTES = 64_000_000


# ---- N > 1 without a launcher: start one ----------------------------------------------------------------------
def relaunch_under_torchrun(n_gpus: int, argv) -> int:
    """`python bench.py --gpus N` (N > 1, no WORLD_SIZE): run the same command under torch.distributed.run, one rank
    per GPU, and print rank 0's JSON line LAST on stdout (anything else the ranks wrote to stdout goes to stderr)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this driver
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for text in proc.stdout.splitlines():
        try:
            if text.startswith("{") and "metric" in json.loads(text):
                if line is not None:
                    print(line, file=sys.stderr)
                line = text
                continue
        except ValueError:
            pass
        print(text, file=sys.stderr)
    sys.stderr.flush()
    if line is not None:
        print(line, flush=True)
    return proc.returncode if proc.returncode else (0 if line is not None else 1)


# ---- the CPU leg ---------------------------------------------------------------------------------------------------
def cpu_reference():
    """(library, kind): the unmodified reference when oracle/_ref/libsela_ref.so travelled with the repo, else the CPU
    restatement.  Checker and CPU baseline only -- nothing of the product path goes through it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import oracle, reference

    impl = reference()
    return (impl, "reference") if impl is not None else (oracle(), "port")


def cpu_baseline(pcm, budget_s=12.0, max_reps=3):
    """Time the CPU path (encode + decode of the same frames) on the host cores: thread fan-out = the reference's
    static contiguous partition over hardware_concurrency() threads (src/sela/encoder.cpp:58-73).  Bounded sample:
    the whole track, repeated until ~budget_s of wall time or max_reps.  Returns (record, blob, offsets, decoded)."""
    impl, kind = cpu_reference()
    cores = os.cpu_count() or 1
    n_frames, n, ch = pcm.shape
    enc_s = dec_s = 0.0
    reps = 0
    t_start = time.time()
    while reps < max_reps and (reps == 0 or time.time() - t_start < budget_s):
        blob, offs, es = impl.encode_frames(pcm, threads=cores)
        dec, ds = impl.decode_frames(blob, offs, ch, threads=cores)
        enc_s += es
        dec_s += ds
        reps += 1
    samples = reps * n_frames * n
    rec = {
        "value": samples / (enc_s + dec_s) / 1e6,
        "unit": "Msamples/s",
        "cores": cores,
        "kind": kind,
        "encode_msps": samples / enc_s / 1e6,
        "decode_msps": samples / dec_s / 1e6,
        "sample": f"{reps} x the full {n_frames}-frame stereo track (rank 0's), encode+decode, {cores} threads "
                  f"(static contiguous frame partition as src/sela/encoder.cpp:58-73)",
    }
    return rec, blob, offs, dec


def _flush_c_stdio():
    import ctypes

    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass


def _newest_profile(name):
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", name)))
    return files[-1] if files else None


def kernel_sources_sha256():
    """SHA-256 over the device sources the library is built from (sela_amd/csrc/*, include/*), file names included.  The
    profile collector (tools/collect_r04.sh) leaves the same digest beside its summaries: a counter file whose digest differs
    from the tree's was collected on other kernels."""
    import glob
    import hashlib

    h = hashlib.sha256()
    for path in sorted(glob.glob(os.path.join(ROOT, "sela_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*"))):
        if os.path.isfile(path):
            h.update(os.path.relpath(path, ROOT).encode() + b"\0")
            with open(path, "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def profiles_state(*sources):
    """{"profiles_stale": bool, ...} for the committed profile files a line quotes: stale = the collector's digest of the kernel
    sources (sources.sha256 in the same directory) is missing or differs from the tree's."""
    now = kernel_sources_sha256()
    dirs = sorted({os.path.dirname(src) for src in sources if src})
    recorded = {}
    for d in dirs:
        try:
            with open(os.path.join(ROOT, d, "sources.sha256")) as f:
                recorded[d] = f.read().split()[0]
        except (OSError, IndexError):
            recorded[d] = None
    return {"profiles_stale": bool(not dirs or any(v != now for v in recorded.values())), "kernel_sources_sha256": now, "recorded": recorded}


def committed_valu_instructions(kernel: str):
    """(instructions per launch, source file): SQ_INSTS_VALU of `kernel` from the newest COMMITTED counter
    summary (profiles/rNN/valu_counters.txt, written by tools/valu_counters.sh) -- not measured in this run."""
    import ast

    path = _newest_profile("valu_counters.txt")
    if not path:
        return None, None
    with open(path) as f:
        for line in f:
            if kernel in line and "SQ_INSTS_VALU" in line:
                try:
                    return float(ast.literal_eval(line[line.index("{"):].strip())["SQ_INSTS_VALU"]), os.path.relpath(path, ROOT)
                except (ValueError, SyntaxError, KeyError):
                    return None, None
    return None, None


def committed_traffic(kernel: str):
    """(HBM bytes per launch, source file, how) of `kernel` from the newest COMMITTED PMC summary (profiles/rNN/traffic.json,
    written by tools/collect_profiles.sh: separate FETCH_SIZE / WRITE_SIZE passes of this same command) -- not measured in
    this run.  `how`: the counters scaled by the factors measured on known-byte kernels (traffic_calibration.json beside it:
    tools/traffic_calib.hip, FETCH_SIZE x 2.0 and WRITE_SIZE x 1.0 at every access width on gfx950), else FETCH doubled per
    MI355X_MICROARCH.md."""
    path = _newest_profile("traffic.json")
    if not path:
        return None, None, None
    with open(path) as f:
        data = json.load(f)
    for name, d in data.items():
        if kernel in name:
            if "hbm_bytes_per_launch_calibrated" in d:
                return d["hbm_bytes_per_launch_calibrated"], os.path.relpath(path, ROOT), "calibrated: " + str(data.get("_calibration", {}).get("file"))
            if "hbm_bytes_per_launch_fetch_x2" in d:
                return d["hbm_bytes_per_launch_fetch_x2"], os.path.relpath(path, ROOT), "FETCH_SIZE doubled (MI355X_MICROARCH.md)"
    return None, None, None


def host_legs(pcm_host, repeats=9):
    """e2e (host-pointer API) and file-to-file numbers from the C++ host (host/sela_filebench), or None."""
    import struct

    exe = os.path.join(ROOT, "host", "sela_filebench")
    if not os.path.exists(exe):
        return None
    scratch = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        wav = os.path.join(tmp, "track.wav")
        data = pcm_host.astype("<i2").tobytes()
        with open(wav, "wb") as f:
            f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt "
                    + struct.pack("<IhHIIHH", 16, 1, CHANNELS, SAMPLE_RATE, SAMPLE_RATE * CHANNELS * 2, CHANNELS * 2, 16)
                    + b"data" + struct.pack("<I", len(data)) + data)
        try:
            out = subprocess.run([exe, wav, tmp, str(repeats)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                return {"error": (out.stderr or out.stdout).strip()[-300:]}
            res = json.loads(out.stdout.strip().splitlines()[-1])
        except (subprocess.TimeoutExpired, ValueError, OSError) as e:
            return {"error": str(e)[-300:]}
    res["files_on"] = "tmpfs (/dev/shm)" if scratch else "the temp directory's file system"
    return res


# ---- the timed machinery ---------------------------------------------------------------------------------------------
class Bench:
    """One process = one rank = one GPU.  Holds what every workload shares: torch, the process group, the barrier."""

    def __init__(self, args):
        import numpy as np
        import torch

        from sela_amd import capi, codec, sharding, synth

        self.np, self.torch, self.capi, self.codec, self.sharding, self.synth = np, torch, capi, codec, sharding, synth
        self.args = args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        assert self.world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={self.world}"
        # SELA_BENCH_RANKS_SHARE_GPU=1 (tests): every rank of an N > 1 run uses GPU 0 and the ranks talk over gloo (RCCL
        # refuses two ranks on one device) -- the whole multi-rank logic of this file on a one-GPU box; not a measurement.
        self.share_gpu = os.environ.get("SELA_BENCH_RANKS_SHARE_GPU") == "1"
        torch.cuda.set_device(0 if self.share_gpu else self.local_rank)
        self.dist = None
        self.coll_device = "cuda"  # where the tensors of the collectives live
        if self.world > 1 or os.environ.get("SELA_BENCH_FORCE_EXCHANGE") == "1":  # (the override runs the N>1 code path on one GPU)
            import torch.distributed as dist

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", str(self.rank))
            os.environ.setdefault("WORLD_SIZE", str(self.world))
            # One node, rendezvous on 127.0.0.1: the bootstrap sockets of RCCL / gloo go over the loopback interface instead of
            # whichever interface the container's hostname resolves to (it may not resolve at all), and a rendezvous that does
            # not complete fails after five minutes instead of the default thirty.
            if os.environ["MASTER_ADDR"] in ("127.0.0.1", "localhost") and os.path.isdir("/sys/class/net/lo"):
                os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
                os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            import datetime

            limit = datetime.timedelta(seconds=300)
            if self.share_gpu:
                dist.init_process_group("gloo", timeout=limit)
                self.coll_device = "cpu"
            else:
                dist.init_process_group("nccl", timeout=limit, device_id=torch.device("cuda", self.local_rank))  # nccl == RCCL on ROCm
            self.dist = dist
            # RCCL prints its version banner through C stdio when the communicator comes up; get it out NOW, on every rank,
            # so that nothing but rank 0's JSON line is left to appear at the end of stdout
            dist.barrier()
            torch.cuda.synchronize()
            _flush_c_stdio()
        self.lib = capi.lib()  # raises if the HIP library is missing: there is no CPU fallback
        self.lib.sela_hip_debug_encode_teams(getattr(args, "encode_teams", -1))
        self.lib.sela_hip_debug_encode_fused(1 if getattr(args, "encode_fused", False) else 0)
        if getattr(args, "priorities", None):
            self.lib.sela_hip_debug_priorities(int(args.priorities.split(":")[0], 16))
        self.lib.sela_hip_debug_encode_split(max(0, getattr(args, "encode_split", 0)))
        self.exchange = torch.cuda.Stream() if self.dist is not None else None
        self.lanes_forced = args.lanes is not None  # (also --lanes=N and abbreviations: argparse's own answer)
        self.n_lanes = max(1, args.lanes if self.lanes_forced else 2)
        # --dump-outputs: the first chain run (the headline's) keeps a sample of its outputs; rank 0's are written
        self.outputs_pending = getattr(args, "dump_outputs", None) is not None and self.rank == 0

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def timed_steps(self, step, steps, after=None):
        """Seconds for exactly `steps` steps run back to back, bracketed by barrier + synchronize, MAX over ranks.  `after`
        runs behind the timed region."""
        torch, dist = self.torch, self.dist
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        self.barrier()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([elapsed], dtype=torch.float64, device=self.coll_device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)  # the same number on every rank
            elapsed = float(t[0].item())
        if after is not None:
            after()
        return elapsed


class ChainJob:
    """A list of HBM-resident batches; a step = every batch through encode -> decode (or decode only), consecutive
    batches (N = 1 track: consecutive steps) on alternating lanes.

    Lanes: consecutive batches are independent chains, so they run on alternating HIP streams with their own buffers:
    the decode of one batch fills the launch tail of the next batch's encode and the other way round.  Everything issued
    inside the timed region completes inside it (device-wide synchronize on both sides); one lane is the strictly serial
    form, reported beside it."""

    def __init__(self, bench: Bench, batches, n_total: int, exchange: bool, pre_encoded=None):
        torch, codec = bench.torch, bench.codec
        self.b, self.batches, self.n_total = bench, batches, n_total
        self.pre = pre_encoded  # decode-only: [(frames, offsets)] per batch, produced outside the timed region
        self.max_batch = max([int(x.shape[0]) for x in batches] + [1])
        self.lanes = []
        n_lanes = bench.n_lanes
        if self.pre is not None and not bench.lanes_forced:
            # Decode-only batches that leave most of the device's wave slots empty (a rank's share of configs[4] on eight
            # GPUs: 2,500 subframe waves where 7 x 1024 fit) are bound by one subframe's latency, not by issue: as many of
            # them in flight as fill the slots once, four at most (the runtime has four hardware queues)
            waves = 2 * self.max_batch
            n_lanes = min(4, max(n_lanes, -(-DECODE_RESIDENT_WAVES // max(waves, 1))))
        for _ in range(n_lanes):
            lane = {"dec": codec.Decoder(self.max_batch, CHANNELS), "stream": torch.cuda.Stream(), "calls": 0, "last": None}
            if self.pre is None:
                lane["enc"] = codec.Encoder(self.max_batch, CHANNELS)
            self.lanes.append(lane)
        self.next_lane = 0
        self.steps_done = 0
        self.outputs = None  # (--dump-outputs: set by run_chain on the headline's job)
        self.exchange = exchange and bench.dist is not None
        if self.exchange:
            ranges = bench.sharding.partition(n_total, bench.world)
            self.max_local = max(e - b for b, e in ranges)
            # two sets in turn: a step's all-gather may still read its set while the next step fills the other
            self.sets = [{"local": torch.zeros(self.max_local, dtype=torch.int64, device="cuda"),
                          "all": torch.zeros(bench.world * self.max_local, dtype=torch.int64, device="cuda"),
                          "done": None} for _ in range(2)]
            self.last_set = None
        self.ring = 0
        self.flag_acc = torch.zeros(8, dtype=torch.int32, device="cuda")  # OR of enc status[0], dec status[0]; max of enc [1], dec [1]

    def streams_overlap(self) -> bool:
        """Do the lanes' streams run side by side?  One spinning workgroup on lane 0, then one on every lane at once."""
        torch = self.b.torch
        if len(self.lanes) < 2 or not hasattr(torch.cuda, "_sleep"):
            return True

        def spin(lanes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for lane in lanes:
                with torch.cuda.stream(lane["stream"]):
                    torch.cuda._sleep(2_000_000)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        spin(self.lanes[:1])
        alone = min(spin(self.lanes[:1]) for _ in range(3))
        together = min(spin(self.lanes) for _ in range(3))
        return together < 1.5 * alone

    def renew_streams(self):
        """New HIP streams for the lanes (the old ones are kept alive, so that the new ones are not the same queues again)."""
        torch = self.b.torch
        torch.cuda.synchronize()
        self.retired = getattr(self, "retired", []) + [lane["stream"] for lane in self.lanes]
        for lane in self.lanes:
            lane["stream"] = torch.cuda.Stream()

    # -- status words: one slot per call, so that nothing a timed call reports is overwritten by the next -------------
    def size_rings(self, steps: int):
        torch = self.b.torch
        self.ring = -(-steps * max(1, len(self.batches)) // len(self.lanes)) + 2
        for lane in self.lanes:
            lane["st_enc"] = torch.zeros((self.ring, 4), dtype=torch.int32, device="cuda")
            lane["st_dec"] = torch.zeros((self.ring, 4), dtype=torch.int32, device="cuda")

    def fold_status(self):
        """OR every slot into the accumulator (between two measurements: outside the timed region) and clear them."""
        torch = self.b.torch
        sh = torch.arange(8, dtype=torch.int32, device="cuda")
        for lane in self.lanes:
            for j, key in enumerate(("st_enc", "st_dec")):
                ring = lane[key]
                bits = ((ring[:, 0:1] >> sh) & 1).amax(dim=0)  # flag bits 0..7, OR over the slots
                self.flag_acc[j] |= (bits << sh).sum().to(torch.int32)
                self.flag_acc[2 + j] = torch.maximum(self.flag_acc[2 + j], ring[:, 1].max())
                ring.zero_()

    def step(self, serial=False, check=None):
        b, torch = self.b, self.b.torch
        ex = self.sets[self.steps_done % 2] if self.exchange else None
        waited = set()
        at = 0
        result = None
        for i, pcm in enumerate(self.batches):
            nb = int(pcm.shape[0])
            li = 0 if serial else self.next_lane % len(self.lanes)
            lane = self.lanes[li]
            self.next_lane += 1
            slot = lane["calls"] % self.ring
            lane["calls"] += 1
            with torch.cuda.stream(lane["stream"]):
                if self.pre is None:
                    out = lane["enc"].encode(pcm, status=lane["st_enc"][slot])
                    frames, offsets = out.frames, out.offsets
                    if ex is not None:
                        if li not in waited and ex["done"] is not None:
                            lane["stream"].wait_event(ex["done"])  # the all-gather of two steps ago has read this set
                        waited.add(li)
                        ex["local"][at: at + nb] = offsets[1:] - offsets[:-1]
                        if i == len(self.batches) - 1:
                            # the path's only exchange: every rank learns the size of every frame of the
                            # job, i.e. where its bytes land in every output file (8 bytes x frames, latency bound -- RCCL
                            # over xGMI).  Decoding does not need the layout, so the collective runs beside the decode on its
                            # own stream; it is complete inside the timed region (device-wide synchronize at its end).
                            for lj in waited:  # (the sizes of the earlier batches were written on the other lanes' streams)
                                b.exchange.wait_stream(self.lanes[lj]["stream"])
                            with torch.cuda.stream(b.exchange):
                                if b.coll_device == "cuda":
                                    b.dist.all_gather_into_tensor(ex["all"], ex["local"])
                                else:  # (the test mode: ranks on one GPU, gloo -- through host memory, synchronously)
                                    gathered = torch.empty(ex["all"].numel(), dtype=torch.int64)
                                    b.dist.all_gather_into_tensor(gathered, ex["local"].cpu())
                                    ex["all"].copy_(gathered)
                                ex["done"] = torch.cuda.Event()
                                ex["done"].record(b.exchange)
                            self.last_set = ex
                else:
                    frames, offsets = self.pre[i]
                back = lane["dec"].decode(frames, offsets, nb, status=lane["st_dec"][slot])
            lane["last"] = (i, nb)
            if check is not None:  # (outside the timed region) status words + round trip + the timed outputs of this batch
                torch.cuda.synchronize()
                check(i, nb, pcm, frames, offsets, back, lane, slot)
            at += nb
            result = (frames, offsets, back)
        self.steps_done += 1
        return result

    def snapshot_lanes(self):
        """What each lane's last (timed) call left in its buffers, cloned: batch index, frame bytes, offsets, PCM."""
        torch = self.b.torch
        torch.cuda.synchronize()
        snaps = []
        for lane in self.lanes:
            if lane["last"] is None:
                continue
            i, nb = lane["last"]
            rec = {"batch": i, "pcm": lane["dec"].pcm[:nb].clone()}
            if self.pre is None:
                offs = lane["enc"].offsets[: nb + 1].clone()
                rec["offsets"] = offs
                rec["frames"] = lane["enc"].frames[: int(offs[-1].item())].clone()
            snaps.append(rec)
        return snaps


def output_sample(np, n_frames: int):
    """The frames --dump-outputs writes the bytes and PCM of: a fixed, seeded draw, the same for every run of the same job."""
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n_frames, size=min(DUMP_FRAMES, n_frames), replace=False))


def keep_outputs(bench: Bench, kept, sample, at: int, nb: int, frames, offsets, back, encoded: bool):
    """Add one batch of a step's outputs to `kept` (host arrays): its frame offsets, continued across batches into offsets of
    the rank's whole stream, and the frame bytes and decoded PCM of the sampled frames among its frames [at, at + nb)."""
    torch, np = bench.torch, bench.np
    sel = torch.as_tensor(sample[(sample >= at) & (sample < at + nb)] - at, dtype=torch.int64, device=back.device)
    kept["pcm"].append(back[sel].cpu().numpy().astype(np.float32))
    if not encoded:  # (decode only: frame bytes and offsets are the job's input, not its output)
        return
    o = offsets[: nb + 1].to(torch.int64)
    kept["offsets"].append(o[1:].cpu().numpy() + kept["stream_bytes"])
    kept["stream_bytes"] += int(o[nb].item())
    starts, lens = o[sel], o[sel + 1] - o[sel]
    pos = torch.arange(int(lens.sum().item()), dtype=torch.int64, device=back.device) + torch.repeat_interleave(starts - (torch.cumsum(lens, 0) - lens), lens)
    kept["bytes"].append(frames[pos].cpu().numpy().astype(np.float32))


def run_chain(bench: Bench, job: ChainJob, steps: int, warmup: int):
    """Warm up, time (all lanes, then one lane), then verify what was timed.  Returns the measurement record."""
    torch, np = bench.torch, bench.np
    job.size_rings(max(steps, warmup, 1))
    # The batches, the codecs' buffers and the status slots were allocated and filled on torch's default stream; the
    # lanes are streams of their own that do not wait for it.  Without this, a lane's first kernels ran while the default
    # stream was still generating the album -- and wrote into memory the allocator had handed out a second time in
    # default-stream order (the sizes of a batch of not-yet-written PCM ended up copied into the album's first frames).
    torch.cuda.synchronize()
    for _ in range(warmup):
        job.step()
    torch.cuda.synchronize()
    job.fold_status()
    # The runtime multiplexes HIP streams onto a few hardware queues, and two lanes that land on ONE queue run one after
    # the other (seen in a process that had created and destroyed streams before): if a probe -- one spinning workgroup
    # per lane -- shows that the lanes' streams do not run side by side, they get new streams before anything is
    # timed (recorded in the line).
    renewals = 0
    while len(job.lanes) > 1 and renewals < 3 and not job.streams_overlap():
        renewals += 1
        job.renew_streams()
        for _ in range(max(2, warmup)):
            job.step()
        torch.cuda.synchronize()
        job.fold_status()
    job.stream_renewals = renewals
    # The first steps after a pause run slow while the clocks settle (a first K-step block of the track ran ~2-3 ms long, at
    # any K): right before the timed region, more untimed steps until WARMUP_SETTLE_S of them have run, in blocks that grow
    # from W to the timed block's K steps (at most SETTLE_BLOCK_S long), so that the device runs as it will when timed.  The
    # block times are agreed over ranks, so that every rank runs as many steps (and collectives).
    settled, settle_steps, block = 0.0, 0, warmup
    while warmup and settled < WARMUP_SETTLE_S:
        t = bench.timed_steps(job.step, block, after=job.fold_status)
        settled += t
        settle_steps += block
        block = max(warmup, min(steps, int(block * SETTLE_BLOCK_S / max(t, 1e-6))))
    timed_s = bench.timed_steps(job.step, steps, after=job.fold_status)
    snaps = job.snapshot_lanes()
    timed_sizes = None
    if job.exchange and job.last_set is not None:  # the layout the LAST TIMED step gathered
        timed_sizes = job.last_set["all"].clone()
    serial_timed_s = bench.timed_steps(lambda: job.step(serial=True), steps, after=job.fold_status) if len(job.lanes) > 1 else timed_s

    # ---- correctness of what was timed -------------------------------------------------------------------------------
    # One more step, serial and synchronised after every batch: its status words, its round trip, and -- batch by batch --
    # equality with what the lanes' last timed calls left behind.  The reference codec is not lossless on every frame
    # (its encoder rounds the prediction half-up, its decoder half-down: a frame whose Q35 sum hits 2^34 mod 2^35 comes
    # back off by one), and parity means reproducing that -- so the round trip may differ from the
    # input in a handful of frames, never in many.  With --dump-outputs, the headline's chain keeps a sample of this step's
    # outputs: those of the last timed step, which they are asserted to equal.
    state = {"lossy": 0, "bytes": 0, "same": True, "compared": 0, "sizes": [], "at": 0}
    n_local = sum(int(x.shape[0]) for x in job.batches)
    kept, sample = None, None
    if bench.outputs_pending:
        bench.outputs_pending = False
        kept, sample = {"pcm": [], "bytes": [], "offsets": [np.zeros(1, np.int64)], "stream_bytes": 0}, output_sample(np, n_local)

    def check(i, nb, pcm, frames, offsets, back, lane, slot):
        dec_st = lane["st_dec"][slot].cpu().numpy().view(np.uint32)
        if int(dec_st[0]) & (bench.capi.FLAG_BAD_FRAME | bench.capi.FLAG_RICE_OVERRUN):
            raise bench.capi.SelaHipError(-5, f"decoder status 0x{int(dec_st[0]):x}")
        state["lossy"] += int((back != pcm).reshape(nb, -1).any(dim=1).sum().item()) if nb else 0
        total = int(offsets[-1].item())
        state["bytes"] += total
        state["sizes"].append((offsets[1:] - offsets[:-1]).clone())
        for s in snaps:
            if s["batch"] != i:
                continue
            same = torch.equal(s["pcm"], back)
            if "frames" in s:
                same = same and torch.equal(s["offsets"], offsets) and torch.equal(s["frames"], frames[:total])
            state["same"] = state["same"] and bool(same)
            state["compared"] += 1
        if kept is not None:
            keep_outputs(bench, kept, sample, state["at"], nb, frames, offsets, back, encoded=job.pre is None)
        state["at"] += nb

    last = job.step(serial=True, check=check)
    torch.cuda.synchronize()
    if timed_sizes is not None and bench.world == 1:  # (one rank: the gathered layout of the last timed step IS this rank's sizes)
        serial_sizes = torch.cat(state["sizes"])
        diff = torch.nonzero(timed_sizes[: serial_sizes.numel()] != serial_sizes).flatten()
        assert diff.numel() == 0, (f"the sizes gathered in the last timed step differ from a serial step's at {diff.numel()} frames: first {diff[:8].tolist()}, "
                                   f"timed {timed_sizes[diff[:8]].tolist()} serial {serial_sizes[diff[:8]].tolist()}")
    job.fold_status()
    acc = job.flag_acc.cpu().numpy().view(np.uint32)
    enc_bad = int(acc[0]) & (bench.capi.FLAG_WORDS_CAP | bench.capi.FLAG_RICE_RANGE | bench.capi.FLAG_COEF_OVERFLOW)
    dec_bad = int(acc[1]) & (bench.capi.FLAG_BAD_FRAME | bench.capi.FLAG_RICE_OVERRUN)
    assert enc_bad == 0 and int(acc[2]) == 0, f"an encode inside the timed region raised flags 0x{int(acc[0]):x} / {int(acc[2])} frames over capacity"
    assert dec_bad == 0 and int(acc[3]) == 0, f"a decode inside the timed region raised flags 0x{int(acc[1]):x} / {int(acc[3])} bad frames"
    assert state["same"] and state["compared"] == len(snaps), "the outputs of the timed (two-lane) steps differ from a serial step's"
    assert state["lossy"] <= max(1, n_local // 500), f"decode(encode(x)) differs from x in {state['lossy']} frames"
    if kept is not None:
        arrays = {}
        if job.pre is None:
            arrays["frame_offsets"] = np.concatenate(kept["offsets"]).astype(np.float64)
            arrays["frame_bytes"] = np.concatenate(kept["bytes"])
        arrays["decoded_pcm"] = np.concatenate(kept["pcm"])
        job.outputs = {"arrays": arrays, "sampled_frames": sample}
    return {
        "step_s": timed_s / steps, "serial_s": serial_timed_s / steps, "timed": {"steps": steps, "timed_s": timed_s, "warmup_steps": warmup, "settle_steps": settle_steps},
        "last": last, "lossy": state["lossy"], "bytes": state["bytes"], "timed_sizes": timed_sizes,
        "timed_outputs": {"status_or_encode": int(acc[0]), "status_or_decode": int(acc[1]), "lanes_compared_with_serial_step": state["compared"],
                          "equal_to_serial_step": bool(state["same"]),
                          "what": "every timed call reports into a status slot of its own, all OR-ed; each lane's last timed outputs (frame bytes, offsets, "
                                  "decoded PCM) compared on the device with a serial synchronised step's"},
    }


def lanes_block(job: ChainJob, m, samples, steps):
    forced = getattr(job.b.args, "priorities", None)
    return {"in_flight": len(job.lanes), "stream_renewals": getattr(job, "stream_renewals", 0),
            "ms_per_step_one_lane": m["serial_s"] * 1e3, "value_one_lane": samples / m["serial_s"] / 1e6,
            "wave_priorities": ("forced " + forced) if forced else "by the library: an encode launch gets the falling schedule when no other stream has library work pending "
                                                                   "(the strictly serial leg), none beside a neighbour (the lanes)",
            "launches_given_the_falling_schedule": int(job.b.lib.sela_hip_debug_launches_alone()),
            "encode_split": {"mode": getattr(job.b.args, "encode_split", 0), "launches_cut_in_two": int(job.b.lib.sela_hip_debug_launches_split()),
                             "what": "experiment (--encode-split N): an encode launch as two halves on two streams, the first half's plan + assemble under the second "
                                     "half's tail; measured slower than the whole launch (DESIGN.md 9), so the library never does it by itself"},
            "what": "consecutive batches are independent encode->decode chains on alternating HIP streams; one lane = strictly serial"}


# ---- workloads -------------------------------------------------------------------------------------------------------
def album_golden():
    with open(os.path.join(ROOT, "tests", "golden", "album_digests.json")) as f:
        return json.load(f)


def gathered_sizes(bench: Bench, all_sizes, n_total: int, max_local: int):
    np = bench.np
    ranges = bench.sharding.partition(n_total, bench.world)
    g = all_sizes.cpu().numpy().reshape(bench.world, max_local)
    return np.concatenate([g[r, : e - b] for r, (b, e) in enumerate(ranges)]).astype("<u8")


def workload_track(bench: Bench, steps: int, warmup: int):
    """configs[1] x N, weak scaling: rank r's track, + the all-gather of the sizes for N > 1."""
    torch, np = bench.torch, bench.np
    frames = bench.synth.frames_for_seconds(TRACK_SECONDS, SAMPLE_RATE)  # 3875
    track = 3 * bench.rank  # the album's 44.1 kHz tracks (tests/golden/album_digests.json holds the reference's digest of each)
    pcm = bench.synth.synth_frames_torch(frames, CHANNELS, track, device="cuda")
    n_total = frames * bench.world
    job = ChainJob(bench, [pcm], n_total, exchange=True)
    m = run_chain(bench, job, steps, warmup)
    out_frames, out_offsets, back = m["last"]
    total = int(out_offsets[-1].item())
    golden = album_golden()["tracks"][track] if track < 100 else None
    # this rank's .sela file and decoded PCM against the reference's digests of the same track
    header = bench.sharding.sela_header(SAMPLE_RATE, 16, CHANNELS, frames)
    blob = out_frames[:total].cpu().numpy()
    digest_ok = None
    if golden is not None and golden["n_frames"] == frames:
        digest_ok = (hashlib.sha256(header + blob.tobytes()).hexdigest() == golden["sela_sha256"]
                     and hashlib.sha256(back.cpu().numpy().tobytes()).hexdigest() == golden["decoded_sha256"])
        assert digest_ok, f"track {track}: .sela / decoded digests differ from the reference's"
    layout_ok = None
    if job.exchange:
        sizes = gathered_sizes(bench, m["timed_sizes"], n_total, job.max_local)
        offs = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))])
        g = album_golden()["tracks"]
        layout_ok = all(15 + int(offs[(r + 1) * frames] - offs[r * frames]) == g[3 * r]["sela_bytes"] for r in range(bench.world))
        mine = sizes[bench.rank * frames: (bench.rank + 1) * frames]
        layout_ok = layout_ok and bool(np.array_equal(mine, np.diff(out_offsets.cpu().numpy().view(np.uint64)).astype("<u8")))
        assert layout_ok, "the gathered frame sizes differ from the reference's file sizes / this rank's own offsets"
    t = torch.tensor([m["lossy"], m["bytes"]], dtype=torch.int64, device=bench.coll_device)
    if bench.dist is not None:
        bench.dist.all_reduce(t)
    samples = n_total * 2048
    rec = {
        "value": samples / m["step_s"] / 1e6, "ms_per_step": m["step_s"] * 1e3, "scaling": "weak",
        "config": {
            "workload": ("BASELINE.json configs[1]: one 3-min 16-bit stereo 44.1 kHz track (3875 frames x 2048 stereo samples) PER GPU, "
                         "encode to .sela frames then decode, bit-exact" + ("; RCCL all-gather of the frame sizes every step" if job.exchange else "")),
            "frames_total": n_total, "frames_rank0": frames, "channels": CHANNELS,
            "sharding": "single track" if bench.world == 1 else f"one track per GPU x{bench.world} (album tracks 0, 3, 6, ...)",
            "batch_frames": frames, "sela_bytes_total": int(t[1].item()), "pcm_bytes_total": n_total * 2048 * CHANNELS * 2,
        },
        "lanes": lanes_block(job, m, samples, steps), "timed": m["timed"], "roundtrip_lossy_frames": int(t[0].item()),
        "layout_matches_reference": layout_ok, "digests_match_reference": digest_ok, "timed_outputs": m["timed_outputs"],
    }
    return rec, job, pcm, (blob, out_offsets.cpu().numpy().view(np.uint64), back.cpu().numpy())


def workload_album(bench: Bench, steps: int, warmup: int):
    """configs[3], strong scaling: this rank's contiguous range of the album's (track, frame) space."""
    torch, np = bench.torch, bench.np
    tracks = bench.synth.album_tracks()
    starts = np.concatenate([[0], np.cumsum([f for _, _, f in tracks])]).astype(np.int64)
    n_total = int(starts[-1])  # 549,365
    my_begin, my_end = bench.sharding.my_range(n_total, bench.rank, bench.world)
    parts = []  # generated on the GPU
    for track, _, frames in tracks:
        b, e = max(my_begin, int(starts[track])), min(my_end, int(starts[track + 1]))
        if b < e:
            parts.append(bench.synth.synth_frames_torch(e - b, CHANNELS, track, first_frame=b - int(starts[track]), device="cuda"))
    local = torch.cat(parts) if parts else torch.zeros((0, 2048, CHANNELS), dtype=torch.int16, device="cuda")
    del parts
    n_batches = max(1, -(-int(local.shape[0]) // ALBUM_BATCH_FRAMES))  # equal batches of <= 65,536 frames
    per_batch = max(1, -(-int(local.shape[0]) // n_batches))
    batches = [local[i: i + per_batch] for i in range(0, local.shape[0], per_batch)] or [local]
    job = ChainJob(bench, batches, n_total, exchange=True)
    m = run_chain(bench, job, steps, warmup)
    layout_ok = None
    if job.exchange:
        # the layout gathered by the last TIMED step must be the one-GPU layout: its digest was computed with the unmodified reference
        golden = album_golden()
        sizes = gathered_sizes(bench, m["timed_sizes"], n_total, job.max_local)
        offs = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))])
        wrong = [t for t in range(len(tracks)) if 15 + int(offs[int(starts[t + 1])] - offs[int(starts[t])]) != golden["tracks"][t]["sela_bytes"]]
        assert not wrong, (f"{len(wrong)} tracks' file sizes differ from the reference's (first: track {wrong[0]}); "
                           f"{int((sizes == 0).sum())} of {len(sizes)} gathered sizes are zero; steps done {job.steps_done}")
        layout_ok = golden.get("frame_sizes_sha256") in (None, hashlib.sha256(sizes.tobytes()).hexdigest())
        assert layout_ok, "the gathered frame-size layout differs from the one-GPU (reference) layout"
    t = torch.tensor([m["lossy"], m["bytes"]], dtype=torch.int64, device=bench.coll_device)
    if bench.dist is not None:
        bench.dist.all_reduce(t)
    samples = n_total * 2048
    rec = {
        "value": samples / m["step_s"] / 1e6, "ms_per_step": m["step_s"] * 1e3, "scaling": "strong", "steps": steps, "warmup": warmup,
        "config": {
            "workload": ("BASELINE.json configs[3]: 100-track synthetic album (34/33/33 tracks at 44.1/48/96 kHz, 549,365 frames x 2048 "
                         f"stereo samples) sharded over {bench.world} GPU(s) in contiguous frame ranges, encode + "
                         + ("RCCL all-gather of the frame sizes + " if job.exchange else "") + "decode"
                         + (", layout checked against the reference's" if job.exchange else "")),
            "frames_total": n_total, "frames_rank0": my_end - my_begin, "channels": CHANNELS, "sharding": f"contiguous frame ranges x{bench.world}",
            "batch_frames": job.max_batch, "sela_bytes_total": int(t[1].item()), "pcm_bytes_total": n_total * 2048 * CHANNELS * 2,
        },
        "lanes": lanes_block(job, m, samples, steps), "timed": m["timed"], "roundtrip_lossy_frames": int(t[0].item()),
        "layout_matches_reference": layout_ok, "timed_outputs": m["timed_outputs"],
        "one_gpu_anchor": "the `album` block (or, with --workload album, the headline) of the --gpus 1 line: same job, one GPU",
    }
    return rec, job, batches[0], None


def workload_decode10k(bench: Bench, steps: int, warmup: int):
    """configs[4], strong scaling, decode only: this rank's contiguous 1/N of 10,000 frames encoded outside the timed region."""
    torch, np = bench.torch, bench.np
    n_total = DECODE10K_FRAMES
    b0, e0 = bench.sharding.my_range(n_total, bench.rank, bench.world)
    pcm = bench.synth.synth_frames_torch(e0 - b0, CHANNELS, DECODE10K_TRACK, first_frame=b0, device="cuda")
    enc = bench.codec.Encoder(max(e0 - b0, 1), CHANNELS)
    out = enc.encode(pcm)
    torch.cuda.synchronize()
    out.check()
    frames, offsets = out.frames, out.offsets
    job = ChainJob(bench, [pcm], n_total, exchange=False, pre_encoded=[(frames, offsets)])
    m = run_chain(bench, job, steps, warmup)
    exact = None
    if bench.rank == 0 and not bench.args.no_cpu_baseline:  # the decode of rank 0's share against the CPU decoder
        impl, kind = cpu_reference()
        f_host, o_host = out.to_host()
        ref_back, _ = impl.decode_frames(f_host, o_host, CHANNELS, threads=os.cpu_count() or 1)
        exact = bool(np.array_equal(ref_back, m["last"][2].cpu().numpy()))
        assert exact, "decode10k: GPU decode differs from the CPU decoder's"
    t = torch.tensor([m["lossy"]], dtype=torch.int64, device=bench.coll_device)
    if bench.dist is not None:
        bench.dist.all_reduce(t)
    samples = n_total * 2048
    share8 = None
    if bench.world == 1:
        # What this workload becomes per GPU on eight of them: rank 0's contiguous eighth (1250 frames), decoded the way a
        # rank would decode it -- same code, same lanes.  One GPU, so a PREDICTION of the eight-GPU line, not a measurement:
        # eight ranks take what the slowest takes, and every rank's share is this size.
        b8, e8 = bench.sharding.my_range(n_total, 0, 8)
        pcm8 = pcm[b8:e8].contiguous()
        enc8 = bench.codec.Encoder(e8 - b8, CHANNELS)
        out8 = enc8.encode(pcm8)
        torch.cuda.synchronize()
        out8.check()
        job8 = ChainJob(bench, [pcm8], e8 - b8, exchange=False, pre_encoded=[(out8.frames, out8.offsets)])
        m8 = run_chain(bench, job8, steps, warmup)
        assert torch.equal(m8["last"][2], m["last"][2][: e8 - b8]), "decode10k: a rank's share decodes differently on its own"
        share8 = {
            "frames": e8 - b8, "ms_per_step": m8["step_s"] * 1e3, "value": (e8 - b8) * 2048 / m8["step_s"] / 1e6,
            "unit": "Msamples/s decode only, ONE GPU on one rank's share of an 8-GPU job",
            "predicted_value_8_gpus": samples / m8["step_s"] / 1e6,
            "predicted_strong_scaling_efficiency_8": m["step_s"] / (8 * m8["step_s"]),
            "what": "rank 0's contiguous 1/8 of the 10,000 frames, timed on this GPU like the full workload; a prediction, not an 8-GPU measurement",
        }
        del job8, enc8, out8
    rec = {
        "value": samples / m["step_s"] / 1e6, "unit": "Msamples/s decode only", "ms_per_step": m["step_s"] * 1e3, "scaling": "strong",
        "per_rank_share_8": share8,
        "steps": steps, "warmup": warmup,
        "config": {
            "workload": (f"BASELINE.json configs[4]: decode-only, {n_total} pre-encoded stereo frames (encoded outside the timed region), "
                         f"every rank decodes its contiguous 1/{bench.world}; no collective"),
            "frames_total": n_total, "frames_rank0": e0 - b0, "channels": CHANNELS, "sharding": f"contiguous frame ranges x{bench.world}",
        },
        "lanes": lanes_block(job, m, samples, steps), "timed": m["timed"], "roundtrip_lossy_frames": int(t[0].item()),
        "bit_exact_vs_cpu_decode": exact, "timed_outputs": m["timed_outputs"],
    }
    return rec, job, pcm, None


def release(bench: Bench):
    """Give a finished workload's device buffers back (the caller has dropped its references)."""
    import gc

    gc.collect()
    bench.torch.cuda.empty_cache()


# ---- per-kernel timing leg (separate from the timed region: events add launch gaps) ---------------------------------
def kernel_leg(bench: Bench, job: ChainJob, pcm0, steps: int):
    np, capi, lib = bench.np, bench.capi, bench.lib
    lib.sela_hip_enable_kernel_timing(1)
    enc, dec = job.lanes[0]["enc"], job.lanes[0]["dec"]
    k_enc, k_dec = [], []
    n0 = int(pcm0.shape[0])
    o2 = enc.encode(pcm0) if n0 else None
    for _ in range(max(5, min(steps, 20)) if n0 else 0):
        # The timed kernel runs where it runs in a step: the encoder behind a decode, the decoder behind an encode, two
        # steps queued so that it starts on a busy, clocked-up device (a launch onto an idle device runs ~10 % slower;
        # an encoder behind an encoder 6 % slower than behind a decoder -- the device's clock follows the power the last
        # kernel drew -- and it is behind a decoder that the rocprofv3 averages of the timed loop see it).
        for _ in range(2):
            dec.decode(o2.frames, o2.offsets, n0)
            o2 = enc.encode(pcm0)
        k_enc.append((capi.kernel_times(3) + [0.0, 0.0])[:3])  # (--encode-fused: one kernel, no plan / assemble)
        for _ in range(2):
            o2 = enc.encode(pcm0)
            dec.decode(o2.frames, o2.offsets, n0)
        k_dec.append(capi.kernel_times(1))
    lib.sela_hip_enable_kernel_timing(0)
    bench.torch.cuda.synchronize()
    return np.array(k_enc), np.array(k_dec), n0, (o2.total_bytes() if o2 is not None else 0)


def kernel_blocks(bench: Bench, k_enc, k_dec, n0: int, sela_bytes0: int, counters_apply: bool):
    """roofline / fp64_valu / valu_issue / kernel_ms of the first batch's launch (rank 0)."""
    enc_blocks_ms = float(k_enc[:, 0].mean())
    pcm_bytes0 = n0 * 2048 * CHANNELS * 2
    algo_bytes = pcm_bytes0 + sela_bytes0  # PCM16 read + .sela frame bytes written, one launch
    achieved = algo_bytes / (enc_blocks_ms * 1e-3) / 1e9
    # which kernel analysed the blocks of this launch: the library picks by launch size (sela_encode.hip, team_lanes_for)
    team_lanes = int(bench.lib.sela_hip_debug_encode_kernel(n0, CHANNELS))
    enc_kernel = f"k_encode_teams<0, {team_lanes}>" if team_lanes else "k_encode_blocks<0, false>"
    traffic, traffic_src, traffic_how = committed_traffic(enc_kernel)
    valu_instr, valu_src = committed_valu_instructions(enc_kernel)
    dec_instr, dec_src = committed_valu_instructions("k_decode_frames<false>")
    if not counters_apply:
        valu_instr = traffic = dec_instr = None  # the committed counter passes are of the single-track launch
    samples0 = n0 * 2048
    enc_ms = float(k_enc.sum(axis=1).mean())
    dec_ms = float(k_dec.sum(axis=1).mean())
    fp64 = FP64_OPS_PER_BLOCK * n0 * 3 / (enc_blocks_ms * 1e-3) / 1e12

    def issue(instr, ms, src, kernel):
        if instr is None:
            return None
        return {
            "kernel": kernel, "achieved": instr / (ms * 1e-3) / 1e9, "peak": VALU_ISSUE_PEAK_GIPS, "unit": "G wave-instructions/s",
            "frac": instr / (ms * 1e-3) / 1e9 / VALU_ISSUE_PEAK_GIPS,
            "instructions_per_launch_from_profiles": instr, "profiles_source": src,
            "note": f"SQ_INSTS_VALU from the committed counter pass named in profiles_source / live kernel time; peak = 1024 SIMDs x {PEAK_CLOCK_GHZ} GHz / 4 cycles per wave64 instruction",
        }

    valu = issue(valu_instr, enc_blocks_ms, valu_src, enc_kernel)
    valu_dec = issue(dec_instr, dec_ms, dec_src, "k_decode_frames<false>")
    return {
        "encode_msps": samples0 / (enc_ms * 1e-3) / 1e6,   # kernels of the first batch, HBM resident
        "decode_msps": samples0 / (dec_ms * 1e-3) / 1e6,
        "encode_target": {"msps": ENCODE_TARGET_MSPS, "met": bool(samples0 / (enc_ms * 1e-3) / 1e6 >= ENCODE_TARGET_MSPS),
                          "ratio": samples0 / (enc_ms * 1e-3) / 1e6 / ENCODE_TARGET_MSPS},
        "kernel_ms": {"encode_blocks": enc_blocks_ms, "encode_blocks_kernel": enc_kernel, "encode_plan": float(k_enc[:, 1].mean()),
                      "encode_assemble": float(k_enc[:, 2].mean()), "decode_frames": dec_ms, "frames_in_launch": n0},
        "fp64_valu": {  # the arithmetic the bit-exact analysis cannot avoid, against the vector FP64 rate
            "achieved": fp64, "peak": FP64_UNFUSED_PEAK_TOPS, "unit": "T unfused FP64 op/s", "frac": fp64 / FP64_UNFUSED_PEAK_TOPS,
        },
        # what binds the kernels in practice: issue slots of the vector ALU (a wave64 instruction takes 4 cycles of a SIMD)
        "valu_issue": valu,
        "valu_issue_decode": valu_dec,
        "profiles": profiles_state(valu_src, traffic_src, dec_src),
        "roofline": {
            "kernel": enc_kernel, "bound": "valu_issue",
            # the HBM figures the contract asks for: algorithmic bytes per launch / live kernel time against the HBM peak
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_from_profiles": traffic_src, "traffic_counters": traffic_how, "algorithmic_bytes_per_launch": algo_bytes,
            # ... and the resource that binds it
            "binding": None if valu is None else {"resource": "valu_issue", "achieved": valu["achieved"], "peak": valu["peak"], "unit": valu["unit"], "frac": valu["frac"]},
            "note": "achieved/peak/frac are the HBM numbers (7 B per stereo sample: the path cannot be HBM bound, SURVEY.md 8(d)); the kernel is bound by "
                    "vector-ALU issue (`binding`, DESIGN.md 5.1); traffic is the committed PMC pass, not this run",
        },
    }


def any_length_leg(np):
    """The any-length / 32-bit route (sela_generic.hip behind sela_hip_encode / sela_hip_decode with samples_per_channel != 2048
    and sela_hip_encode_i32 / sela_hip_decode_i32), host pointers in and out, on frames the fast kernels do not take: lightly tuned,
    not part of `value` -- the line says what the route costs and that its bytes are the oracle's (the checker, as in
    cpu_baseline)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import oracle
    from sela_amd import codec
    from sela_amd.synth import synth_pcm

    out = {"what": "host pointers in and out, synchronous calls, best of 3 (the first call of a kind also loads its kernels and grows the thread's "
                   "scratch); the any-length kernels -- the fast kernels' loops with a run-time length, one wave per block (sela_generic.hip) and the fast "
                   "decoder's lane-parallel parse and synthesis with 32-bit samples, by segments beyond 2048 samples (k_decode_subframes32); checked against the oracle"}
    o = oracle()

    def best(fn):
        times, res = [], None
        for _ in range(3):
            t0 = time.perf_counter()
            res = fn()
            times.append(time.perf_counter() - t0)
        return min(times), res

    for label, n, nf in (("stereo_4096_samples", 4096, 64), ("stereo_1000_samples", 1000, 256)):
        pcm = synth_pcm(n * nf, 2, 21).reshape(nf, n, 2)
        t_enc, (frames, offs) = best(lambda: codec.encode_host(pcm))
        t_dec, back = best(lambda: codec.decode_host(frames, offs, 2))
        want = b"".join(o.frame_encode(pcm[f]) for f in range(nf))
        ok = frames.tobytes() == want and bool(np.array_equal(back, pcm.reshape(-1, 2)))
        assert ok, "the any-length route differs from the oracle"
        out[label] = {"frames": nf, "encode_ms": t_enc * 1e3, "decode_ms": t_dec * 1e3, "encode_msps": n * nf / t_enc / 1e6,
                      "decode_msps": n * nf / t_dec / 1e6, "bit_exact_vs_oracle": ok}
    wide = np.clip(2 * synth_pcm(2048 * 32, 2, 22).astype(np.int32).reshape(32, 2048, 2).transpose(0, 2, 1) + 1, -65535, 65535)
    wide = np.ascontiguousarray(wide)
    t_enc, (frames, offs) = best(lambda: codec.encode_i32(wide))
    t_dec, dec = best(lambda: codec.decode_i32(frames, offs, 2))
    ok = frames.tobytes() == b"".join(o.frame_encode_i32(np.ascontiguousarray(wide[f])) for f in range(32))
    assert ok, "the 32-bit route differs from the oracle"
    out["stereo_2048_samples_17_bit"] = {"frames": 32, "encode_ms": t_enc * 1e3, "decode_ms": t_dec * 1e3, "bit_exact_vs_oracle": ok,
                                         "lossless": bool(all(np.array_equal(np.stack(dec[f]), wide[f]) for f in range(32)))}
    return out


def write_outputs(path: str, outputs, np):
    """--dump-outputs: DIR/<name>.npy for every kept array, float32 / float64 (exact for the bytes, samples and offsets)."""
    arrays = outputs["arrays"]
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_BUDGET_BYTES, f"--dump-outputs: {total} bytes, over the {DUMP_BUDGET_BYTES} allowed"
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {
        "dir": os.path.abspath(path), "bytes": total, "arrays": {name: {"shape": list(a.shape), "dtype": str(a.dtype)} for name, a in arrays.items()},
        "sampled_frames": int(len(outputs["sampled_frames"])), "seed": DUMP_SEED,
        "what": "rank 0's outputs of the headline's last timed step: frame_offsets = every frame's offset in the rank's frame stream (+ its end), "
                "frame_bytes = the bytes of the sampled frames back to back, decoded_pcm = their decoded samples [frame, sample, channel]; the frames "
                "are a seeded draw of the rank's frames, in order (decode-only workloads: decoded_pcm alone)",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["track", "album", "decode10k"], default=None,
                    help="the headline workload (default: track = one 3-min track per GPU, weak scaling; album and decode10k then ride along as extra blocks)")
    ap.add_argument("--no-extra-legs", action="store_true", help="headline only (profiling runs)")
    ap.add_argument("--extra-steps", type=int, default=3, help="steps per measurement of the album block")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-legs", action="store_true")
    ap.add_argument("--lanes", type=int, default=None, help="(default 2) batches in flight: independent encode->decode chains on their own HIP streams")
    ap.add_argument("--encode-teams", type=int, default=-1, choices=[-1, 0, 8, 16],
                    help="experiments only: force the encoder's block kernel (0: k_encode_blocks, 8 / 16: k_encode_teams); -1: the library's own choice by launch size")
    ap.add_argument("--priorities", type=str, default=None,
                    help="experiments only: the team kernel's wave priorities by quarters of a wave's work (hex, e.g. 00010203: falling from 3 to 0)")
    ap.add_argument("--encode-split", type=int, default=0,
                    help="experiments only: 1..999 cuts every encode launch of teams of 16 in two (that share per mille to the first half); 0 (default): never")
    ap.add_argument("--encode-fused", action="store_true",
                    help="experiments only: the encoder's one-launch form (the host pipeline's) on device pointers, no plan / assemble kernels")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the headline's last timed step computed to DIR/<name>.npy (rank 0; a seeded sample of the frames)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(args.gpus, sys.argv[1:]))

    bench = Bench(args)
    np, torch = bench.np, bench.torch
    headline = args.workload or "track"
    runners = {"track": workload_track, "album": workload_album, "decode10k": workload_decode10k}

    rec, job, pcm0, host_out = runners[headline](bench, args.steps, args.warmup)
    dumped = write_outputs(args.dump_outputs, job.outputs, np) if job.outputs is not None else None
    kern = None
    if headline != "decode10k":
        k_enc, k_dec, n0, sela0 = kernel_leg(bench, job, pcm0, args.steps)
        if bench.rank == 0:
            kern = kernel_blocks(bench, k_enc, k_dec, n0, sela0, counters_apply=headline == "track")
    result = None
    if bench.rank == 0:
        result = {
            "metric": METRIC, "value": rec["value"], "unit": rec.get("unit", "Msamples/s"), "n_gpus": bench.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": rec["scaling"], "vs_baseline": None,
            "dtype": "f64+int64", "data": "synthetic",
        }
        result.update({k: v for k, v in rec.items() if k not in ("value", "unit", "ms_per_step", "scaling", "steps", "warmup")})
        if kern is not None:
            result.update(kern)
            result["profiles_stale"] = kern["profiles"]["profiles_stale"]
        if dumped is not None:
            result["dump_outputs"] = dumped
    pcm_host = None
    if headline == "track" and bench.rank == 0:
        pcm_host = pcm0.cpu().numpy()
    del job, pcm0
    release(bench)

    # ---- the other workloads as extra blocks -------------------------------------------------------------------------
    if args.workload is None and not args.no_extra_legs:
        for name, steps, warmup in (("album", args.extra_steps, 1), ("decode10k", args.steps, args.warmup)):
            extra, j, p, _ = runners[name](bench, steps, warmup)
            if bench.rank == 0:
                result[name] = extra
            del j, p
            release(bench)

    if bench.rank == 0 and headline == "track":
        if bench.world == 1 and not args.no_host_legs:
            legs = host_legs(pcm_host.reshape(-1, CHANNELS))
            if legs is not None and "error" not in legs:
                result["e2e"] = {"encode_ms": legs["e2e_encode_ms"], "decode_ms": legs["e2e_decode_ms"],
                                 "encode_msps": legs["e2e_encode_msps"], "decode_msps": legs["e2e_decode_msps"],
                                 "what": "sela_hip_encode / sela_hip_decode on page-locked host buffers: H2D + kernels + D2H, steady_clock, median of %d" % legs["repeats"]}
                result["file_to_file"] = {"encode_ms": legs["file_encode_ms"], "decode_ms": legs["file_decode_ms"],
                                          "encode_msps": legs["file_encode_msps"], "decode_msps": legs["file_decode_msps"],
                                          "equals_e2e_bytes": legs["file_equals_e2e"], "files_on": legs["files_on"],
                                          "what": "sela::encodeFile / decodeFile on paths (the reference's `sela -e` / `-d`, src/main.cpp:29-41): reader threads, "
                                                  "H2D, kernels, D2H, writer threads overlapped; in-process, HIP initialised"}
                if "play_first_packet_ms" in legs:
                    result["file_to_file"]["play"] = {"first_packet_ms": legs["play_first_packet_ms"], "all_packets_ms": legs["play_all_ms"],
                                                      "what": "sela::Player::playFile (the reference's `sela -p`, src/sela/player.cpp:30-104) into a sink that "
                                                              "compares the packets with the decoded file: call -> first packet, call -> last packet"}
            else:
                result["e2e"] = result["file_to_file"] = legs
        if not args.no_cpu_baseline:
            # rank 0 times the reference on ITS track (bounded: ~12 s at N = 1, ~5 s beside waiting ranks); the CPU output
            # doubles as the checker of what the GPU produced in the serial step the timed outputs were compared with
            base, blob, offs, dec = cpu_baseline(pcm_host, budget_s=12.0 if bench.world == 1 else 5.0, max_reps=3 if bench.world == 1 else 2)
            g_frames, g_offsets, g_back = host_out
            base["bit_exact_vs_gpu"] = bool(np.array_equal(blob, g_frames) and np.array_equal(offs, g_offsets) and np.array_equal(dec, g_back))
            result["cpu_baseline"] = base
            assert base["bit_exact_vs_gpu"], "GPU output differs from the CPU reference"
            if bench.world == 1:
                # (still the cpu_baseline leg -- the only place bench.py touches oracle/: the any-length route is timed and then
                # checked against the oracle's bytes, like the headline against the reference's)
                result["any_length"] = any_length_leg(np)
    if bench.dist is not None:
        bench.dist.barrier()
        bench.dist.destroy_process_group()
    _flush_c_stdio()  # RCCL prints its version banner through C stdio; keep the JSON line the LAST line of stdout
    if bench.rank == 0:
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
