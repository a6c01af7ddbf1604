"""Time of the inference-time frame encoder (model.models._conv_stack in eval mode) from raw
128 x 128 frames, hipEvents around each line (nfdpf.prof.EventPair), one process:

  (a) loop     the loop DPF._frame_encodings runs without the HIP encoder: T calls of B = 64
               frames through PyTorch/MIOpen, stacked;
  (b) batched  one PyTorch/MIOpen call on all B T frames;
  (c) hip      nfdpf.ops.frame_encoder (csrc/frame_enc.hip);
  (d) DPF.filtering_pos from frames at the C2 shape (64 rows x 1000 particles x 50 steps), with
      NFDPF_HIP_ENCODER=0 and =1,

at H = 32 and 192 and at 64 frames (one step's batch: B = 64, T = 1) and 3 200 frames (the C2
pass's: B = 64, T = 50).  The first MIOpen call and the first HIP call of the process are timed
with a host clock around a synchronise before anything else runs (MIOpen's first-use search /
the code object's load); then every line of a case is warmed up, and each round times one run of
each line in turn, so drift of the device's clocks falls on all of them alike.  One JSON line per
line and case, appended to the output file as it is measured: median, min and max in ms, and for
the HIP lines the time over the 73.7 MFLOP-per-frame floor at the 157.3 TFLOP/s FP32 peak.

    python scripts/frame_encoder_time.py [OUT.jsonl] [REPS]   (default profiles/frame_encoder_time.jsonl, 20)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT]
import torch  # noqa: E402

WARM = 3
MFLOP_PER_FRAME = 2e-6 * (4096 * 16 * 48 + 1024 * 32 * 256 + 256 * 64 * 512 + 64 * 128 * 1024 + 16 * 256 * 2048)
PEAK_TFLOPS = 157.3


def floor_ms(frames, H):
    return frames * (MFLOP_PER_FRAME + 2e-6 * 4096 * H) * 1e6 / (PEAK_TFLOPS * 1e12) * 1e3


def timed(lines, reps, dev):
    from nfdpf.prof import EventPair
    for _ in range(WARM):
        for run in lines:
            run()
    torch.cuda.synchronize()
    ms = [[] for _ in lines]
    for _ in range(reps):
        for i, run in enumerate(lines):
            ev = EventPair()
            ev.record_start(dev)
            run()
            ev.record_end(dev)
            ms[i].append(ev.ms())
            ev.close()
    return ms


def main():
    import model.models as mm
    from nfdpf import _lib, ops
    from nfdpf.pack import frame_encoder_tensors
    _lib.load()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frame_encoder_time.jsonl")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    out = open(out_path, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    g = torch.Generator().manual_seed(1)
    B, T = 64, 50
    obs = torch.rand(B, T, 3, 128, 128, generator=g).to(dev)
    torch.cuda.synchronize()

    def encoder(H):
        torch.manual_seed(2)
        enc = mm._conv_stack(H)
        with torch.no_grad():
            for m in enc:
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0.0, 0.2)
                    m.running_mean.uniform_(0.0, 0.5)
                    m.running_var.uniform_(0.5, 2.0)
        enc = enc.to(dev).eval()
        blob = torch.cat([t.reshape(-1).float() for t in frame_encoder_tensors(enc)]).to(dev)
        return enc, blob

    def loop(enc, n_t):
        with torch.no_grad():
            return torch.stack([enc(obs[:, t].float()) for t in range(n_t)], dim=1)

    def batched(enc, n_t):
        with torch.no_grad():
            return enc(obs[:, :n_t].reshape(-1, 3, 128, 128)).view(B, n_t, -1)

    # first calls of the process, host clock around a synchronise
    enc, blob = encoder(32)
    t0 = time.perf_counter()
    ops.frame_encoder(blob, obs[:, :1], 32)
    torch.cuda.synchronize()
    emit(what="first_call", line="hip", H=32, frames=B, ms=(time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    loop(enc, 1)
    torch.cuda.synchronize()
    emit(what="first_call", line="miopen", H=32, frames=B, ms=(time.perf_counter() - t0) * 1e3)

    for H in (32, 192):
        enc, blob = encoder(H)
        for n_t in (1, T):
            frames = B * n_t
            lines = [lambda: loop(enc, n_t), lambda: batched(enc, n_t),
                     lambda: ops.frame_encoder(blob, obs[:, :n_t], H)]
            t0 = time.perf_counter()
            ref, bat, hip = [run() for run in lines]
            torch.cuda.synchronize()
            settle = (time.perf_counter() - t0) * 1e3
            err = float((hip - ref).abs().max()), float((bat - ref).abs().max())
            ms = timed(lines, reps, dev)
            for name, v in zip(("loop", "batched", "hip"), ms):
                rec = dict(what="encoder", line=name, H=H, frames=frames, B=B, T=n_t, ms_median=statistics.median(v),
                           ms_min=min(v), ms_max=max(v), reps=reps)
                if name == "hip":
                    rec.update(floor_ms=floor_ms(frames, H), over_floor=statistics.median(v) / floor_ms(frames, H),
                               over_loop=statistics.median(v) / statistics.median(ms[0]),
                               max_abs_diff_vs_loop=err[0])
                if name == "batched":
                    rec.update(max_abs_diff_vs_loop=err[1])
                if name == "loop":
                    rec.update(first_round_all_lines_ms=settle)
                emit(**rec)

    # (d) filtering_pos from frames at the C2 shape
    from arguments import parse_args
    from DPFs import DPF
    a = parse_args([])
    a.NF_dyn, a.NF_cond, a.measurement, a.resampler_type = True, True, "cos", "soft"
    a.hiddensize, a.num_particles, a.batchsize, a.sequence_length = 32, 1000, B, T
    torch.manual_seed(3)
    dpf = DPF(a).to(dev).eval()
    start = torch.cat([torch.rand(B, 2, generator=g) * 100, torch.randn(B, 2, generator=g)], 1).to(dev)
    vel = torch.randn(B, T, 2, generator=g).to(dev)

    def filt(flag):
        def run():
            os.environ["NFDPF_HIP_ENCODER"] = flag
            with torch.no_grad():
                return dpf.filtering_pos(obs, start, vel)
        return run
    ms = timed([filt("0"), filt("1")], reps, dev)
    for flag, v in zip(("0", "1"), ms):
        emit(what="filtering_pos", NFDPF_HIP_ENCODER=flag, H=32, B=B, N=1000, T=T, frames=B * T,
             ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), reps=reps)
    out.close()


if __name__ == "__main__":
    main()
