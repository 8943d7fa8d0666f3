"""TorchScript export CLI (reference /root/reference/export.py:99-152).

python export.py --model-load WEIGHTS/check_point_100.pth [arch flags]

Uses build_parser (NOT get_arguments): arch flags must be passed manually,
matching the reference contract. Produces jit_traced_model_cpu.pth and (when
a GPU is present) jit_traced_model_gpu.pth in --save-path, consumed by the
in-repo C++ LibTorch app (tools/cpp_infer). With ``--raw-input`` (and a
GPU) it also saves jit_traced_model_gpu_raw.pth, which takes one raw
(H,W,3) uint8 frame of any size, resizes and normalises it on the device
(bit-identical to the Python evaluation's Pillow resize) and returns the boxes
in the frame's own pixels (tools/cpp_infer ``-r``). ``--infer-dtype bf16``
or ``fp8`` traces the GPU files on the bf16 / e4m3 kernels and saves them
with a ``_bf16`` / ``_fp8`` suffix (the CPU file stays fp32). ``--serve``
(GPU and kernel extension) also saves jit_traced_model_gpu_serve[_bf16|_fp8]
.pth: raw frame in, one packed (1+N, 6) detection tensor out, nothing inside
that blocks graph capture (tools/cpp_infer ``-g``).
"""

import torch

from real_time_helmet_detection_amd.config import build_parser
from real_time_helmet_detection_amd.engine.trainer import load_network
from real_time_helmet_detection_amd.engine.exporter import (
    build_export_module, build_serve_module, export_model)

if __name__ == '__main__':
    args = build_parser()
    device = torch.device('cpu')
    network, _, _, _ = load_network(args, device)
    predictor = build_export_module(args, network)
    serve = None
    if args.serve:
        serve = build_serve_module(args, network, args.imsize or 512)
    export_model(predictor, save_dir=args.save_path,
                 imsize=args.imsize or 512,
                 raw_input=getattr(args, 'raw_input', False),
                 pretrained=args.pretrained,
                 infer_dtype=args.infer_dtype, serve=serve)
