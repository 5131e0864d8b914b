import sys, ctypes as C, torch
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch
cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 1234, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)
eng = m.engine; lib = eng.lib; V = cfg.vocab
eng.begin_sequence(1024, [V-4, V-3, V-2, V-1])
eng.prefill(torch.randn(440, cfg.hidden, device="cuda"), row=0)
eng.prefill(torch.randn(110, cfg.hidden, device="cuda"), row=1)
eng.stream.synchronize()
with torch.cuda.stream(eng.stream):
    lens0 = eng.lens.clone()
    L.check(lib.vv_graph_begin(eng.sp), "b"); eng._seq_A(V-4, V-2); ge = C.c_void_p(); L.check(lib.vv_graph_end(eng.sp, C.byref(ge)), "e")
    for _ in range(12):
        lib.vv_graph_launch(ge, eng.sp)
        eng.lens.copy_(lens0)
    eng.stream.synchronize()
