"""The seven device-call classes of sela_amd.codec share one base (_DeviceCall); what their callers see stays: the public methods
and every parameter of them, the constructors' included, as they were before the classes were folded.  No GPU, no library call."""
import inspect

from sela_amd import codec

INIT = "(self, max_frames: 'int', channels: 'int', stride: 'int', device=None)"
CHECK, COUNT, FALLBACK = "(self) -> 'None'", "(self) -> 'int'", "(self, n_frames=None) -> 'int'"
DECODE, PAYLOAD = "(self, frames, offsets, n_frames: 'int')", "(self, payload, max_frames=None)"

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
}


def test_the_classes_keep_their_methods_and_parameters():
    for name, want in SIGNATURES.items():
        cls = getattr(codec, name)
        got = {m: str(inspect.signature(f)) for m, f in inspect.getmembers(cls, inspect.isfunction) if m == "__init__" or not m.startswith("_")}
        assert got == want, name
        assert cls.__doc__ and cls.__doc__.startswith("sela_hip_"), name
