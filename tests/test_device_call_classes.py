"""The seven device-call classes of sela_amd.codec share one base (_DeviceCall), the two window decoders another (_WindowCall)
and the two whole-track encoders a third (_WholeEncode); what their callers see stays: the public methods and every parameter
of them, the constructors' included, as they were before the classes were folded.  No GPU, no library call."""
import inspect

from sela_amd import codec

INIT = "(self, max_frames: 'int', channels: 'int', stride: 'int', device=None)"
CHECK, COUNT, FALLBACK = "(self) -> 'None'", "(self) -> 'int'", "(self, n_frames=None) -> 'int'"
DECODE, PAYLOAD = "(self, frames, offsets, n_frames: 'int')", "(self, payload, max_frames=None)"
WINDOWS, PACK = "(self, frames, offsets, n_frames_total: 'int', windows)", "(starts, first_frames, n_frames) -> 'np.ndarray'"

SIGNATURES = {
    "Decoder32": {"__init__": INIT, "check": CHECK, "decode": DECODE, "decode_payload": PAYLOAD},
    "DecoderN": {"__init__": INIT, "check": CHECK, "decode": DECODE, "decode_payload": PAYLOAD, "route": COUNT},
    "Verifier": {"__init__": INIT, "check": CHECK, "lossy_frames": COUNT, "route": COUNT, "verify": "(self, frames, offsets, n_frames: 'int', pcm)",
                 "verify_payload": "(self, payload, pcm, max_frames=None)"},
    "Leveler": {"__init__": INIT, "check": CHECK, "loud_frames": COUNT, "measure": DECODE, "measure_payload": PAYLOAD,
                "records": "(levels) -> 'np.ndarray'", "route": COUNT},
    "Leveler32": {"__init__": INIT, "check": CHECK, "fallback_frames": FALLBACK, "loud_frames": COUNT, "measure": DECODE, "measure_payload": PAYLOAD,
                  "records": "(levels) -> 'np.ndarray'"},
    "Verifier32": {"__init__": INIT, "check": CHECK, "fallback_frames": FALLBACK, "lossy_frames": COUNT,
                   "verify": "(self, frames, offsets, n_frames: 'int', samples, lengths=None)",
                   "verify_payload": "(self, payload, samples, lengths=None, max_frames=None)"},
    "VerifierPcm": {"__init__": "(self, max_frames: 'int', channels: 'int', stride: 'int', bytes_per_sample: 'int', device=None)", "check": CHECK,
                    "fallback_frames": FALLBACK, "lossy_frames": COUNT, "verify": "(self, frames, offsets, n_frames: 'int', pcm, pcm_samples=None)",
                    "verify_payload": "(self, payload, pcm, pcm_samples=None, max_frames=None)"},
    "WindowDecoder": {"__init__": "(self, max_windows: 'int', window_samples: 'int', channels: 'int', planar_float: 'bool' = False, device=None, whole: 'bool' = False)",
                      "check": CHECK, "decode": WINDOWS, "pack": PACK},
    "WindowDecoder32": {"__init__": "(self, max_windows: 'int', window_samples: 'int', channels: 'int', format: 'int', sample_bits: 'int' = 24, device=None, whole: 'bool' = False)",
                        "check": CHECK, "decode": WINDOWS, "pack": PACK, "wide_samples": COUNT},
    "WholeEncoder": {"__init__": "(self, max_samples: 'int', channels: 'int', lossless: 'bool' = False, device=None, capacity=None)", "check": CHECK,
                     "encode": "(self, pcm)", "to_host": "(self)"},
    "WholeEncoderPcm": {"__init__": "(self, max_samples: 'int', channels: 'int', bytes_per_sample: 'int', lossless: 'bool' = False, capacity=None, device=None)",
                        "check": CHECK, "encode": "(self, pcm, n_samples=None)", "needed_bytes": COUNT, "to_host": "(self)"},
    "WholeDecoder": {"__init__": "(self, max_frames: 'int', channels: 'int', device=None, capacity=None)", "check": CHECK,
                     "decode": "(self, frames, offsets, n_frames: 'int', capacity=None)", "decode_payload": "(self, payload, max_frames=None, capacity=None)",
                     "route": COUNT},
}


def test_the_classes_keep_their_methods_and_parameters():
    for name, want in SIGNATURES.items():
        cls = getattr(codec, name)
        got = {m: str(inspect.signature(f)) for m, f in inspect.getmembers(cls, inspect.isfunction) if m == "__init__" or not m.startswith("_")}
        assert got == want, name
        assert cls.__doc__ and cls.__doc__.startswith("sela_hip_"), name
