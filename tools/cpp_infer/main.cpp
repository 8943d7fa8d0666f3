// Standalone C++ inference app (the reference's PytorchToCpp equivalent,
// README.md:65-79 — in-repo this time).
//
// Loads a TorchScript model traced by export.py (jit_traced_model_cpu.pth /
// jit_traced_model_gpu.pth) plus an image, runs detection, prints the boxes
// and reports FPS over --iters runs.
//
//   ./helmet_infer -m jit_traced_model_gpu.pth -i image.jpg [-n 100]
//
// The app depends only on LibTorch: images are binary PPM (P6), the
// zero-dependency format every tool can emit (`convert img.jpg img.ppm`,
// or `python tools/cpp_infer/to_ppm.py img.jpg`). Preprocessing matches
// utils.imload in layout only: resize to 512x512, scale to [0,1], ImageNet
// normalize. The resize here is at::upsample_bilinear2d, a plain 2-tap
// filter WITHOUT antialiasing, while the Python path (Pillow BILINEAR) widens
// its filter with the ratio on a downscale: for a frame larger than the
// network input this app feeds the network different pixels than the Python
// evaluation did.
//
//   ./helmet_infer -r -m jit_traced_model_gpu_raw.pth -k <_C*.so> -i image.ppm
//
// -r closes that gap: the PPM goes to the model as the uint8 HWC tensor it
// was read into, the raw-input trace (export.py --raw-input) resizes and
// normalises it on the device bit-identically to the Python path, and the
// boxes are printed in the source image's pixels. GPU only; -s is unused
// (the size is baked into the trace).
//
//   ./helmet_infer [-g] -m jit_traced_model_gpu_serve[_bf16|_fp8].pth \
//       -k <_C*.so> -i image.ppm
//
// A serving model (export.py --serve) is recognised by its output: ONE
// packed (1+N, 6) float tensor instead of a tuple — row 0 [count, 0...],
// rows 1..count [x1 y1 x2 y2 score class] in the frame's pixels. It takes
// the raw frame like -r. Each iteration copies the frame from pinned host
// memory into a static device input, runs the model, copies the packed
// tensor back to pinned host memory and synchronises; the FPS includes both
// copies. Plain, the model runs by forward. With -g the forward is captured
// once into a device graph (three warm-up forwards on a side stream first,
// so the conv variant choice and the TorchScript executor have settled) and
// replayed per iteration. If the capture throws, the app
// reports it and exits non-zero.
// When the traced GPU model embeds the native gfx950 ops (torch.ops.rthd.*,
// the default export.py GPU trace), pass the kernel extension with
// -k <path to real_time_helmet_detection_amd/ops/_C*.so>; it is dlopen'd
// before torch::jit::load so the rthd:: custom ops resolve.
#include <torch/script.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/HIPGraph.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/StreamGuard.h>
#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

static torch::Tensor read_ppm(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open image: " + path);
  char magic[3] = {};
  int w = 0, h = 0, maxv = 0;
  if (fscanf(f, "%2s", magic) != 1 || strcmp(magic, "P6") != 0)
    throw std::runtime_error("image must be binary PPM (P6): " + path);
  // skip comments/whitespace
  auto read_int = [&]() {
    int c;
    do {
      c = fgetc(f);
      if (c == '#') { while (c != '\n' && c != EOF) c = fgetc(f); }
    } while (isspace(c) || c == '#');
    int v = 0;
    while (isdigit(c)) { v = v * 10 + (c - '0'); c = fgetc(f); }
    return v;
  };
  w = read_int();
  h = read_int();
  maxv = read_int();
  if (w <= 0 || h <= 0 || maxv != 255)
    throw std::runtime_error("unsupported PPM: " + path);
  std::vector<unsigned char> buf((size_t)w * h * 3);
  if (fread(buf.data(), 1, buf.size(), f) != buf.size())
    throw std::runtime_error("truncated PPM: " + path);
  fclose(f);
  return torch::from_blob(buf.data(), {h, w, 3}, torch::kUInt8).clone();
}

static torch::Tensor load_image(const std::string& path, int imsize) {
  auto img = read_ppm(path);
  img = img.permute({2, 0, 1}).to(torch::kFloat32).div_(255.0).unsqueeze(0);
  img = at::upsample_bilinear2d(img, {imsize, imsize},
                                /*align_corners=*/false);
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
  for (int c = 0; c < 3; ++c)
    img[0][c] = (img[0][c] - mean[c]) / stdv[c];
  return img;
}

static const char* kNames[] = {"hat", "person"};

// detections of a packed (1+N, 6) host tensor
static void print_packed(const torch::Tensor& packed) {
  auto p = packed.contiguous();
  const float* d = p.data_ptr<float>();
  const int64_t n = p.size(0) - 1;
  const int64_t count = std::min<int64_t>(std::max<int64_t>((int64_t)d[0], 0),
                                          n);
  const int nshow = (int)std::min<int64_t>(count, 20);
  printf("%lld detections (showing %d)\n", (long long)count, nshow);
  for (int i = 0; i < nshow; ++i) {
    const float* r = d + (int64_t)(1 + i) * 6;
    const int cls = (int)r[5];
    printf("det %2d: %-7s score %.3f box [%7.1f %7.1f %7.1f %7.1f]\n", i,
           cls >= 0 && cls < 2 ? kNames[cls] : "?", r[4], r[0], r[1], r[2],
           r[3]);
  }
}

// serving model: frame is the (H,W,3) uint8 host tensor
static int run_serving(torch::jit::script::Module& model,
                       const torch::Tensor& frame, torch::Device device,
                       int iters, bool graph_mode) {
  auto host_in = frame.pin_memory();
  auto static_in = torch::empty_like(frame, frame.options().device(device));
  // everything below runs on a stream of our own: a capture may not use the
  // default stream
  // (the generic guard and the device-wide synchronise: the HIP-specific
  // ones are inline calls into the HIP runtime, which this app does not link
  // — see CMakeLists.txt; nothing else runs on the device here)
  auto stream = c10::hip::getStreamFromPoolMasqueradingAsCUDA();
  c10::StreamGuard guard(stream.unwrap());
  static_in.copy_(host_in, /*non_blocking=*/true);

  torch::Tensor out;
  for (int i = 0; i < 3; ++i) out = model.forward({static_in}).toTensor();
  at::hip::device_synchronize();
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 6 &&
                  out.scalar_type() == torch::kFloat32,
              "serving model: expected a packed (1+N, 6) float tensor");

  at::cuda::CUDAGraph graph;
  if (graph_mode) {
    try {
      graph.capture_begin();
      out = model.forward({static_in}).toTensor();
      graph.capture_end();
    } catch (const std::exception& e) {
      std::cerr << "helmet_infer: graph capture failed: " << e.what() << "\n";
      return 2;
    }
  }
  auto host_out = torch::empty(
      out.sizes(), out.options().device(torch::kCPU).pinned_memory(true));

  auto step = [&]() {
    static_in.copy_(host_in, /*non_blocking=*/true);
    if (graph_mode)
      graph.replay();
    else
      out = model.forward({static_in}).toTensor();
    host_out.copy_(out, /*non_blocking=*/true);
    at::hip::device_synchronize();
  };
  step();
  print_packed(host_out);

  for (int i = 0; i < 10; ++i) step();
  auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) step();
  auto t1 = std::chrono::steady_clock::now();
  const double sec = std::chrono::duration<double>(t1 - t0).count();
  printf("%d iters in %.3f s -> %.1f FPS, raw %lldx%lld frame, serving "
         "model, %s (gpu)\n", iters, sec, iters / sec,
         (long long)frame.size(1), (long long)frame.size(0),
         graph_mode ? "graph replay, frame upload and result download "
                      "included"
                    : "plain forward, frame upload and result download "
                      "included");
  return 0;
}

static int run(int argc, char** argv) {
  std::string model_path, image_path, kernels_path;
  int iters = 100, imsize = 512;
  bool raw = false, graph_mode = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "-r")) { raw = true; continue; }
    if (!strcmp(argv[i], "-g")) { graph_mode = true; continue; }
    if (i >= argc - 1) break;  // every other flag takes a value
    if (!strcmp(argv[i], "-m")) model_path = argv[++i];
    else if (!strcmp(argv[i], "-i")) image_path = argv[++i];
    else if (!strcmp(argv[i], "-k")) kernels_path = argv[++i];
    else if (!strcmp(argv[i], "-n")) iters = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-s")) imsize = atoi(argv[++i]);
  }
  if (model_path.empty() || image_path.empty()) {
    std::cerr << "usage: " << argv[0]
              << " -m model.pth -i image.ppm [-k rthd_ops.so] [-n iters]"
                 " [-s imsize] [-r] [-g]\n";
    return 1;
  }
  if (!kernels_path.empty()) {
    // the kernel extension links libtorch_python, which expects the CPython
    // symbols to be present in the process (normally exported by the python
    // binary) — provide them via libpython before loading the extension.
    dlopen("libpython3.10.so.1.0", RTLD_NOW | RTLD_GLOBAL);
    if (!dlopen(kernels_path.c_str(), RTLD_NOW | RTLD_GLOBAL))
      throw std::runtime_error(std::string("dlopen failed: ") + dlerror());
  }

  torch::jit::script::Module model = torch::jit::load(model_path);
  model.eval();
  const bool cuda = torch::cuda::is_available() &&
                    model_path.find("gpu") != std::string::npos;
  torch::Device device(cuda ? torch::kCUDA : torch::kCPU);
  model.to(device);

  // a serving model takes the raw frame too; its file name says so, its
  // output (a tensor, no tuple) confirms it
  const bool serve_name =
      model_path.find("gpu_serve") != std::string::npos;
  if ((raw || serve_name || graph_mode) && !cuda)
    throw std::runtime_error("-r, -g and serving models need a GPU and a "
                             "jit_traced_model_gpu_raw / _gpu_serve model");
  torch::NoGradGuard ng;
  if (serve_name) {
    auto frame = read_ppm(image_path);
    auto probe = model.forward({frame.to(device)});
    if (probe.isTensor())
      return run_serving(model, frame, device, iters, graph_mode);
    throw std::runtime_error("model named gpu_serve returns no tensor");
  }
  if (graph_mode)
    throw std::runtime_error("-g replays serving models only "
                             "(jit_traced_model_gpu_serve*.pth)");
  auto img = raw ? read_ppm(image_path).to(device)
                 : load_image(image_path, imsize).to(device);

  auto first = model.forward({img});
  if (first.isTensor())
    throw std::runtime_error("this model returns a packed tensor: it is a "
                             "serving model, keep gpu_serve in its name");
  auto out = first.toTuple();
  auto boxes = out->elements()[0].toTensor().cpu();
  auto clss = out->elements()[1].toTensor().cpu();
  auto scores = out->elements()[2].toTensor().cpu();
  const char* const* names = kNames;
  const int nshow = std::min<int64_t>(boxes.size(0), 20);
  printf("%lld detections (showing %d)\n", (long long)boxes.size(0), nshow);
  for (int i = 0; i < nshow; ++i) {
    const int cls = clss[i].item<int64_t>();
    printf("det %2d: %-7s score %.3f box [%7.1f %7.1f %7.1f %7.1f]\n", i,
           cls < 2 ? names[cls] : "?", scores[i].item<float>(),
           boxes[i][0].item<float>(), boxes[i][1].item<float>(),
           boxes[i][2].item<float>(), boxes[i][3].item<float>());
  }

  // FPS: warmup 10 then timed iters
  for (int i = 0; i < 10; ++i) model.forward({img});
  if (cuda) at::hip::device_synchronize();
  auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) model.forward({img});
  if (cuda) at::hip::device_synchronize();
  auto t1 = std::chrono::steady_clock::now();
  const double sec = std::chrono::duration<double>(t1 - t0).count();
  if (raw)
    printf("%d iters in %.3f s -> %.1f FPS, raw %lldx%lld frame, "
           "preprocess included (gpu)\n", iters, sec, iters / sec,
           (long long)img.size(1), (long long)img.size(0));
  else
    printf("%d iters in %.3f s -> %.1f FPS @ %dx%d (%s)\n", iters, sec,
           iters / sec, imsize, imsize, cuda ? "gpu" : "cpu");
  return 0;
}

int main(int argc, char** argv) {
  try {
    return run(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << "helmet_infer: " << e.what() << "\n";
    return 1;
  }
}
