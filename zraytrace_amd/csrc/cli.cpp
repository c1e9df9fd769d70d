// cli.cpp — `zrt-raytrace`: main.zig's command line on the HIP path.
//
//   zrt-raytrace width height samples depth scene_index filename
//
// A plain client of libzrt.so's C ABI (as a Zig host would be): builds the
// scene (scenes.zig:267-277 via zrt_scene_load), renders it with zrt_render
// (raytrace.zig:136-203: BVH on, DefaultPrng seed 42 -> counter RNG), prints
// the reference's start, per-scanline and summary lines on stderr
// (raytrace.zig:143-159, 37-50 + 184, 191-201) and writes the PNG (main.zig:33,
// png_image.zig:96-148).  The scanline lines carry each row's counters as the
// reference counts them (ZRT_FLAG_SCANLINES, zrt_render_progress); they are
// printed when the frame is done (it is one launch), and their Pixels/s is the
// frame's rate, since rows are not rendered one after another.  Assets come from $ZRT_ASSETS, else <exe dir>/../assets;
// $ZRT_DEVICE picks the GPU, $ZRT_DEVICES="0,1,..." renders over several
// (zrt_render_multi: tiles round-robin, one RCCL gather).  $ZRT_PASS_SAMPLES=N renders
// progressively (zrt_render_progressive, passes of N samples rounded up to whole
// sample chunks; 0: the library's default): one line per pass on stderr in place
// of the scanline lines, and the PNG rewritten after every pass - the final PNG
// and the summary's counters are those of a run without the variable.
// $ZRT_ADAPTIVE_TOL=<t> renders with adaptive sampling (zrt_render_adaptive: 8x8 tiles
// that have converged within t stop early; $ZRT_ADAPTIVE_FIRST = the first level's
// samples, default one chunk): one line per level, then the scanline lines once, from the
// rows accumulated over the levels (a row's samples are its tiles' own), and
// $ZRT_ADAPTIVE_MAP=<file.png> receives the sample-count map as a grey PNG (samples / cap).
// $ZRT_DENOISE=1 filters the frame with the default a-trous filter (zrt_render_denoised;
// $ZRT_DENOISE=iters,sigma_color,sigma_normal,sigma_albedo,sigma_depth sets it explicitly):
// the PNG is the denoised frame, $ZRT_DENOISE_NOISY=<file.png> also receives the
// unfiltered one.  It composes with $ZRT_ADAPTIVE_TOL (no level or scanline lines then,
// and no sample map) and is refused with $ZRT_DEVICES or $ZRT_PASS_SAMPLES.
// $ZRT_DENOISE_VARIANCE=1 beside $ZRT_DENOISE selects the variance-guided filter
// (zrt_render_denoised_guided; $ZRT_DENOISE=1: its own defaults), =2 adds albedo
// demodulation; the samples must then be two or more whole sample chunks
// ($ZRT_SAMPLE_CHUNK sets params.sample_chunk, default 32).
// $ZRT_TEMPORAL_FRAMES=n renders a sequence of n frames through the temporal step and the
// guided filter (zrt_render_temporal, both at their defaults; the samples as for
// $ZRT_DENOISE_VARIANCE) and writes the last filtered frame; $ZRT_TEMPORAL_TRUCK=<delta>
// (default 0: a static camera) moves the camera sideways: frame k's origin and
// lower_left_corner are the scene's plus (float(k) * delta) * horizontal per component, in
// f32.  One line per frame on stderr in place of the scanline lines.  It is refused with
// every other mode above.
// $ZRT_AO_SAMPLES=n [$ZRT_AO_RADIUS=r] $ZRT_AO_OUT=<file.png> also writes the frame's
// ambient-occlusion plane (zrt_render_ao: n rays per pixel, radius r, default +inf) as a
// grey PNG, beside any mode above; the frame's own output is unchanged.
// $ZRT_PANORAMA_OUT=<file.png> [$ZRT_PANORAMA_WIDTH=w, default 512] also writes a w x w/2
// equirectangular panorama from the scene camera's origin (zrt_rays_equirect + zrt_radiance,
// with the run's samples, depth, seed, PRNG and traversal), beside any mode above.
// $ZRT_LENS=pinhole|thin|ortho|equirect|fisheye $ZRT_LENS_OUT=<file.png> [$ZRT_APERTURE=a, default 0]
// [$ZRT_FOCUS_DIST=d, default: the camera's own plane] [$ZRT_FISHEYE_FOV=degrees, default 180]
// also writes the frame through that lens at the scene camera's pose (zrt_lens_from_camera +
// zrt_render_lens over the whole width x height, with the run's samples, depth, seed, PRNG and
// traversal), beside any mode above.  pinhole is the scene camera itself over the whole width.
// The two go together, and the three options only with them: a run that sets any of the five
// without both ZRT_LENS and ZRT_LENS_OUT is refused before anything is rendered.
// $ZRT_LENS_DENOISE=plain|guided|demod (with ZRT_LENS and ZRT_LENS_OUT, refused without them):
// ZRT_LENS_OUT receives the lens frame filtered (zrt_render_lens_denoised over the whole frame) by
// the default a-trous filter, the default variance-guided filter without, or with, albedo
// demodulation.  The guided ones need the samples to be two or more whole sample chunks.
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zrt.h"

namespace {

// std.fmt.parseInt(u16, s, 10)
bool parse_u16(const char* s, uint16_t* out, const char** err) {
  if (!s) {
    *err = "missing argument";
    return false;
  }
  const char* p = s;
  if (*p == '+') ++p;
  if (!*p) {
    *err = "InvalidCharacter";
    return false;
  }
  uint32_t v = 0;
  for (; *p; ++p) {
    if (*p < '0' || *p > '9') {
      *err = "InvalidCharacter";
      return false;
    }
    v = v * 10 + uint32_t(*p - '0');
    if (v > 0xffff) {
      *err = "Overflow";
      return false;
    }
  }
  *out = uint16_t(v);
  return true;
}

std::string default_assets() {
  if (const char* env = std::getenv("ZRT_ASSETS")) return env;
  char buf[4096];
  const ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
  if (n <= 0) return "assets";
  buf[n] = 0;
  std::string exe(buf);
  return exe.substr(0, exe.rfind('/')) + "/../assets";
}

const char* scene_title(unsigned index) {  // the scene constructors' first line
  switch (index) {
    case 0: return "Rendering scene Man and a big ball";            // scenes.zig:27
    case 1: return "Rendering scene Three balls";                   // scenes.zig:55
    case 2: return "Rendering scene Bunny and a big ball";          // scenes.zig:103
    case 3: return "Rendering scene Bunny and a big ball";          // scenes.zig:207 (sic)
    case 4: return "Rendering scene Bunny and a circle of balls";   // scenes.zig:169 (sic)
    case 6: return "Rendering scene Textured teapot (config C5 substitute)";
    default: return nullptr;                                        // goat prints none
  }
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// $ZRT_PASS_SAMPLES: the preview after every pass of zrt_render_progressive
struct Preview {
  const char* filename;
  uint32_t width, height;
  uint64_t pixels;  // rendered: x < height (raytrace.zig:168)
};
int on_pass(void* user, const float* rgb, const zrt_pass_info* info) {
  const Preview* pv = static_cast<const Preview*>(user);
  // (the pass's rays are not counted per pass: camera rays / s is the rate a pass can report)
  std::fprintf(stderr, "Pass: %u samples done (+%u) Changed pixels: %llu Max change: %.6g Msamples/s: %.2f\n",
               info->samples_done, info->pass_samples, (unsigned long long)info->changed_pixels,
               double(info->max_abs_change),
               double(pv->pixels) * info->pass_samples / (double(info->render_ms) / 1000.0) / 1e6);
  // (an unwritable preview stops the run; the final write below reports the error)
  return zrt_image_write_png(pv->filename, rgb, pv->width, pv->height) != ZRT_OK;
}

int on_frame(void*, const float*, uint32_t frame) {
  std::fprintf(stderr, "Frame: %u\n", frame + 1);
  return 0;
}

int on_level(void*, const float*, const zrt_level_info* info) {
  std::fprintf(stderr, "Level: %u samples Tiles: %u Still active: %u Samples: %llu Changed pixels: %llu "
                       "Max change: %.6g Msamples/s: %.2f\n",
               info->level_samples, info->tiles_rendered, info->tiles_active_after,
               (unsigned long long)info->samples_rendered, (unsigned long long)info->changed_pixels,
               double(info->max_abs_change), double(info->samples_rendered) / (double(info->render_ms) / 1000.0) / 1e6);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  std::fprintf(stderr, "raytrace\nUSAGE;\nraytrace width heigth samples depth scene_index filename\n");
  uint16_t width = 0, height = 0, samples = 0, depth = 0, scene_index = 0;
  const char* err = nullptr;
  uint16_t* fields[5] = {&width, &height, &samples, &depth, &scene_index};
  for (int i = 0; i < 5; ++i) {
    if (!parse_u16(i + 1 < argc ? argv[i + 1] : nullptr, fields[i], &err)) {
      std::fprintf(stderr, "error: %s\n", err);
      return 1;
    }
  }
  if (argc < 7) {
    std::fprintf(stderr, "error: missing argument\n");
    return 1;
  }
  const char* filename = argv[6];

  const auto t_start = std::chrono::steady_clock::now();
  if (const char* title = scene_title(scene_index)) std::fprintf(stderr, "%s\n", title);
  zrt_scene_data* data = nullptr;
  zrt_camera camera;
  int rc = zrt_scene_load(scene_index, default_assets().c_str(), &data, &camera);
  if (rc != ZRT_OK) {
    std::fprintf(stderr, "error: %s\n", zrt_last_error());
    return 1;
  }
  const zrt_scene* scene = zrt_scene_view(data);

  zrt_params params;
  std::memset(&params, 0, sizeof(params));
  params.width = width;
  params.height = height;
  params.samples_per_pixel = samples;
  params.max_depth = depth;
  params.bounded_volume_hierarchy = 1;  // main.zig:28
  params.rng_mode = ZRT_RNG_COUNTER;
  params.prng = ZRT_PRNG_XOROSHIRO128;
  params.traversal = ZRT_TRAVERSAL_FAST;
  params.seed = 42;  // DefaultPrng.init(42) in every scene
  params.world_size = 1;
  if (const char* dev = std::getenv("ZRT_DEVICE")) params.device = uint32_t(std::atoi(dev));
  if (const char* chunk = std::getenv("ZRT_SAMPLE_CHUNK")) params.sample_chunk = uint32_t(std::strtoul(chunk, nullptr, 10));
  // $ZRT_DEVICES="0,1,...,7": tiles over those GPUs, one RCCL gather (zrt_render_multi)
  std::vector<uint32_t> devices;
  if (const char* list = std::getenv("ZRT_DEVICES")) {
    for (const char* q = list; *q;) {
      char* end = nullptr;
      const unsigned long d = std::strtoul(q, &end, 10);
      if (end == q) break;
      devices.push_back(uint32_t(d));
      q = *end == ',' ? end + 1 : end;
    }
  }

  const char* pass_env = std::getenv("ZRT_PASS_SAMPLES");
  if (pass_env && !devices.empty()) {
    std::fprintf(stderr, "error: ZRT_PASS_SAMPLES renders on one GPU: unset ZRT_DEVICES (or ZRT_PASS_SAMPLES)\n");
    zrt_scene_free(data);
    return 1;
  }

  const char* tol_env = std::getenv("ZRT_ADAPTIVE_TOL");
  if (tol_env && (pass_env || !devices.empty())) {
    std::fprintf(stderr, "error: ZRT_ADAPTIVE_TOL renders on one GPU, not in plain passes: unset ZRT_DEVICES and "
                         "ZRT_PASS_SAMPLES (or ZRT_ADAPTIVE_TOL)\n");
    zrt_scene_free(data);
    return 1;
  }

  // $ZRT_DENOISE=1 (the defaults) or iters,sigma_color,sigma_normal,sigma_albedo,sigma_depth: the
  // output file is the a-trous-filtered frame (zrt_render_denoised); $ZRT_DENOISE_NOISY=path
  // also writes the unfiltered one
  const char* dn_env = std::getenv("ZRT_DENOISE");
  const char* var_env = dn_env ? std::getenv("ZRT_DENOISE_VARIANCE") : nullptr;
  uint32_t dn_flags = 0;
  zrt_denoise dn;
  if (dn_env) {
    if (pass_env || !devices.empty()) {
      std::fprintf(stderr, "error: ZRT_DENOISE filters a frame rendered on one GPU, not in plain passes: unset "
                           "ZRT_DEVICES and ZRT_PASS_SAMPLES (or ZRT_DENOISE)\n");
      zrt_scene_free(data);
      return 1;
    }
    if (var_env) {
      const int v = std::atoi(var_env);
      if (v != 1 && v != 2) {
        std::fprintf(stderr, "error: ZRT_DENOISE_VARIANCE is 1 (variance-guided) or 2 (with albedo demodulation)\n");
        zrt_scene_free(data);
        return 1;
      }
      uint32_t default_flags = 0;
      zrt_denoise_guided_defaults(&dn, &default_flags);
      dn_flags = v == 2 ? uint32_t(ZRT_DN_DEMODULATE) : 0u;
    } else {
      zrt_denoise_defaults(&dn);
    }
    if (std::strchr(dn_env, ',')) {
      unsigned iters = 0;
      if (std::sscanf(dn_env, "%u,%f,%f,%f,%f", &iters, &dn.sigma_color, &dn.sigma_normal, &dn.sigma_albedo,
                      &dn.sigma_depth) != 5) {
        std::fprintf(stderr, "error: ZRT_DENOISE is 1 or iterations,sigma_color,sigma_normal,sigma_albedo,sigma_depth\n");
        zrt_scene_free(data);
        return 1;
      }
      dn.iterations = iters;
    }
  }

  // $ZRT_TEMPORAL_FRAMES=n [$ZRT_TEMPORAL_TRUCK=delta]: n frames through zrt_render_temporal
  const char* tf_env = std::getenv("ZRT_TEMPORAL_FRAMES");
  std::vector<zrt_camera> cameras;
  if (tf_env) {
    if (pass_env || tol_env || dn_env || !devices.empty()) {
      std::fprintf(stderr, "error: ZRT_TEMPORAL_FRAMES renders its own sequence on one GPU: unset ZRT_DEVICES, "
                           "ZRT_PASS_SAMPLES, ZRT_ADAPTIVE_TOL and ZRT_DENOISE (or ZRT_TEMPORAL_FRAMES)\n");
      zrt_scene_free(data);
      return 1;
    }
    const unsigned long n = std::strtoul(tf_env, nullptr, 10);
    const char* truck = std::getenv("ZRT_TEMPORAL_TRUCK");
    const float delta = truck ? std::strtof(truck, nullptr) : 0.0f;
    if (n == 0 || n > 65535) {
      std::fprintf(stderr, "error: ZRT_TEMPORAL_FRAMES is a frame count, 1 .. 65535\n");
      zrt_scene_free(data);
      return 1;
    }
    for (unsigned long k = 0; k < n; ++k) {
      zrt_camera ck = camera;
      const float f = float(k) * delta;
      ck.origin.x = camera.origin.x + f * camera.horizontal.x;
      ck.origin.y = camera.origin.y + f * camera.horizontal.y;
      ck.origin.z = camera.origin.z + f * camera.horizontal.z;
      ck.lower_left_corner.x = camera.lower_left_corner.x + f * camera.horizontal.x;
      ck.lower_left_corner.y = camera.lower_left_corner.y + f * camera.horizontal.y;
      ck.lower_left_corner.z = camera.lower_left_corner.z + f * camera.horizontal.z;
      cameras.push_back(ck);
    }
  }

  // $ZRT_AO_SAMPLES=n [$ZRT_AO_RADIUS=r] $ZRT_AO_OUT=file.png: also write the AO plane; the
  // settings are checked here, before anything is rendered (zrt_debug_ao_plan: no device)
  const char* ao_n = std::getenv("ZRT_AO_SAMPLES");
  const char* ao_out = std::getenv("ZRT_AO_OUT");
  zrt_ao ao;
  std::memset(&ao, 0, sizeof(ao));
  zrt_params ao_params = params;
  ao_params.flags = 0;
  ao_params.rank = 0;
  ao_params.world_size = 1;
  if (ao_n || ao_out || std::getenv("ZRT_AO_RADIUS")) {
    if (!ao_n || !ao_out) {
      std::fprintf(stderr, "error: the AO plane needs both ZRT_AO_SAMPLES=<rays per pixel> and ZRT_AO_OUT=<file.png>\n");
      zrt_scene_free(data);
      return 1;
    }
    char* end = nullptr;
    const unsigned long n = std::strtoul(ao_n, &end, 10);
    const char* r = std::getenv("ZRT_AO_RADIUS");
    char* rend = nullptr;
    ao.radius = r ? std::strtof(r, &rend) : HUGE_VALF;
    if (r && (*rend != '\0' || rend == r)) ao.radius = NAN;  // not a number: refused below
    ao.n_samples = (*end != '\0' || end == ao_n || n > 0xffffffffUL) ? 0u : uint32_t(n);
    zrt_ao_plan plan;
    if (zrt_debug_ao_plan(&ao_params, &ao, 1, &plan) != ZRT_OK) {
      std::fprintf(stderr, "error: ZRT_AO_SAMPLES is 1 .. 1024 rays per pixel, ZRT_AO_RADIUS a length > 0.001 (%s)\n",
                   zrt_last_error());
      zrt_scene_free(data);
      return 1;
    }
  }

  // $ZRT_PANORAMA_OUT=file.png [$ZRT_PANORAMA_WIDTH=w]: also write a panorama; checked here,
  // before anything is rendered (zrt_debug_radiance_plan: no device)
  const char* pano_out = std::getenv("ZRT_PANORAMA_OUT");
  uint32_t pano_w = 512;
  struct zrt_radiance pano_rq;
  std::memset(&pano_rq, 0, sizeof(pano_rq));
  pano_rq.n_samples = samples;
  if (pano_out || std::getenv("ZRT_PANORAMA_WIDTH")) {
    const char* w = std::getenv("ZRT_PANORAMA_WIDTH");
    char* end = nullptr;
    const unsigned long v = w ? std::strtoul(w, &end, 10) : pano_w;
    zrt_radiance_plan plan;
    if (!pano_out || (w && (*end != '\0' || end == w)) || v < 2 || v > 16384 || v % 2 != 0 ||
        zrt_debug_radiance_plan(&ao_params, &pano_rq, uint32_t(v * (v / 2)), 1, 0, &plan) != ZRT_OK) {
      std::fprintf(stderr, "error: the panorama needs ZRT_PANORAMA_OUT=<file.png>, an even ZRT_PANORAMA_WIDTH of 2 .. 16384 "
                           "and one sample or more\n");
      zrt_scene_free(data);
      return 1;
    }
    pano_w = uint32_t(v);
  }

  // $ZRT_LENS=<model> $ZRT_LENS_OUT=file.png [$ZRT_APERTURE, $ZRT_FOCUS_DIST, $ZRT_FISHEYE_FOV]: also
  // write the frame through a lens; checked here, before anything is rendered (no device)
  const char* lens_name = std::getenv("ZRT_LENS");
  const char* lens_out = std::getenv("ZRT_LENS_OUT");
  zrt_lens lens;
  zrt_camera_query lens_q;
  std::memset(&lens_q, 0, sizeof(lens_q));
  lens_q.w = width;
  lens_q.h = height;
  lens_q.n_samples = samples;
  const char* lens_dn = std::getenv("ZRT_LENS_DENOISE");
  uint32_t lens_dn_mode = 3;  // 0 plain, 1 guided, 2 guided with demodulation
  if (lens_name || lens_out || lens_dn || std::getenv("ZRT_APERTURE") || std::getenv("ZRT_FOCUS_DIST") ||
      std::getenv("ZRT_FISHEYE_FOV")) {
    const char* names[] = {"pinhole", "thin", "ortho", "equirect", "fisheye"};
    uint32_t kind = 5;
    for (uint32_t k = 0; k < 5 && lens_name; ++k)
      if (std::strcmp(lens_name, names[k]) == 0) kind = k;
    bool ok = lens_name && lens_out && kind < 5;
    float opt[3] = {0.0f, 0.0f, 180.0f};  // aperture, focus distance (0: the camera's plane), fisheye field of view
    const char* opt_names[3] = {"ZRT_APERTURE", "ZRT_FOCUS_DIST", "ZRT_FISHEYE_FOV"};
    for (int k = 0; k < 3; ++k)
      if (const char* e = std::getenv(opt_names[k])) {
        char* end = nullptr;
        opt[k] = std::strtof(e, &end);
        if (end == e || *end != '\0' || !(opt[k] >= 0.0f)) ok = false;
      }
    if (lens_dn) {
      const char* modes[] = {"plain", "guided", "demod"};
      for (uint32_t k = 0; k < 3; ++k)
        if (std::strcmp(lens_dn, modes[k]) == 0) lens_dn_mode = k;
      zrt_variance_plan vp;
      if (lens_dn_mode > 2 || (lens_dn_mode > 0 && zrt_debug_variance_plan(&ao_params, samples, &vp) != ZRT_OK)) ok = false;
    }
    zrt_camera_plan plan;
    if (!ok || zrt_lens_from_camera(kind, &camera, opt[0], opt[1], opt[2], &lens) != ZRT_OK ||
        zrt_debug_camera_plan(&ao_params, &lens_q, 1, 0, &plan) != ZRT_OK) {
      std::fprintf(stderr, "error: the lens frame needs ZRT_LENS=pinhole|thin|ortho|equirect|fisheye and ZRT_LENS_OUT=<file.png>; "
                           "ZRT_APERTURE and ZRT_FOCUS_DIST are lengths >= 0, ZRT_FISHEYE_FOV degrees > 0; ZRT_LENS_DENOISE=plain|guided|demod "
                           "(guided, demod: the samples must be two or more whole sample chunks)\n");
      zrt_scene_free(data);
      return 1;
    }
  }

  std::fprintf(stderr, "Raytrace start\n");
  std::fprintf(stderr, " - Surfaces:                 %u\n", scene->n_prims);
  std::fprintf(stderr, " - Pixels:                   %ux%u\n", unsigned(width), unsigned(height));
  std::fprintf(stderr, " - Samples per pixel:        %u\n", unsigned(samples));
  std::fprintf(stderr, " - Recursion depth:          %u\n", unsigned(depth));
  std::fprintf(stderr, " - Bounded volume hierarchy: true\n");
  std::fprintf(stderr, scene->n_prims > 10 ? "Using Bounded Volume Hierarchy\n" : "Using surface list\n");

  std::vector<float> image(size_t(width) * height * 3, 0.0f);
  std::vector<zrt_scanline> rows(height);
  zrt_stats stats;
  const auto t_render = std::chrono::steady_clock::now();
  std::vector<uint32_t> sample_map;
  std::vector<float> noisy;
  double denoise_ms = 0.0;
  if (tf_env) {
    zrt_denoise_guided_defaults(&dn, &dn_flags);
    rc = zrt_render_temporal(scene, cameras.data(), uint32_t(cameras.size()), &params, nullptr, &dn, dn_flags,
                             on_frame, nullptr, image.data(), &stats);
  } else if (dn_env) {
    zrt_adaptive ad;
    std::memset(&ad, 0, sizeof(ad));
    if (tol_env) ad.tolerance = std::strtof(tol_env, nullptr);
    if (const char* first = std::getenv("ZRT_ADAPTIVE_FIRST")) ad.first_level = uint32_t(std::strtoul(first, nullptr, 10));
    noisy.assign(image.size(), 0.0f);
    if (var_env)
      rc = zrt_render_denoised_guided(scene, &camera, &params, tol_env ? &ad : nullptr, &dn, dn_flags, image.data(),
                                      noisy.data(), nullptr, nullptr, &stats, &denoise_ms);
    else
      rc = zrt_render_denoised(scene, &camera, &params, tol_env ? &ad : nullptr, &dn, image.data(), noisy.data(),
                               nullptr, &stats, &denoise_ms);
  } else if (tol_env) {
    zrt_adaptive ad;
    std::memset(&ad, 0, sizeof(ad));
    ad.tolerance = std::strtof(tol_env, nullptr);
    if (const char* first = std::getenv("ZRT_ADAPTIVE_FIRST")) ad.first_level = uint32_t(std::strtoul(first, nullptr, 10));
    sample_map.assign(size_t(width) * height, 0u);
    rc = zrt_render_adaptive_progress(scene, &camera, &params, &ad, on_level, nullptr, image.data(),
                                      sample_map.data(), &stats, rows.data());
  } else if (pass_env) {
    const Preview pv{filename, width, height, uint64_t(height) * height};
    rc = zrt_render_progressive(scene, &camera, &params, uint32_t(std::strtoul(pass_env, nullptr, 10)), on_pass,
                                const_cast<Preview*>(&pv), image.data(), &stats);
  } else if (devices.empty()) {
    rc = zrt_render_progress(scene, &camera, &params, image.data(), &stats, rows.data());
  } else {
    params.flags |= ZRT_FLAG_SCANLINES;
    zrt_multi* multi = nullptr;
    rc = zrt_multi_create(scene, &params, devices.data(), uint32_t(devices.size()), &multi);
    if (rc == ZRT_OK) rc = zrt_multi_render(multi, &camera, &params, image.data(), &stats);
    if (rc == ZRT_OK) rc = zrt_multi_scanlines(multi, rows.data(), height);
    const std::string msg = zrt_last_error();
    zrt_multi_destroy(multi);
    if (rc != ZRT_OK) std::fprintf(stderr, "error: %s\n", msg.c_str());
  }
  if (rc != ZRT_OK) {
    if (devices.empty()) std::fprintf(stderr, "error: %s\n", zrt_last_error());
    zrt_scene_free(data);
    return 1;
  }
  const double runtime = seconds_since(t_start);
  const double call = seconds_since(t_render);
  const double render_runtime = stats.render_ms / 1000.0;  // the sampling loop itself
  std::fprintf(stderr, "Preprocess time: %.2f seconds\n", runtime - render_runtime);
  // printProgress after every scanline (raytrace.zig:37-50, 184)
  const double pixels_per_second = double(stats.pixels_processed) / render_runtime;
  unsigned long long pixels = 0, samples_sum = 0, rays = 0;
  for (uint32_t y = 0; y < height && !pass_env && !dn_env && !tf_env; ++y) {
    pixels += rows[y].pixels;
    samples_sum += rows[y].samples;
    rays += rows[y].rays;
    std::fprintf(stderr,
                 "Scanline: %u/%u Pixels: %llu Samples: %llu Rays: %llu Recursion limit: %llu Reflections: %llu "
                 "Background hits: %llu Pixels/s: %.1f\n",
                 y + 1, unsigned(height), pixels, samples_sum, rays,
                 (unsigned long long)rows[y].recursion_depth_hits, (unsigned long long)rows[y].reflections,
                 (unsigned long long)rows[y].background_hits, pixels_per_second);
  }
  std::fprintf(stderr, "Rendering ready\n");
  std::fprintf(stderr, "  Total reflections:     %llu\n", (unsigned long long)stats.reflections);
  std::fprintf(stderr, "  Total background hits: %llu\n", (unsigned long long)stats.background_hits);
  std::fprintf(stderr, "  Total pixels:          %llu\n", (unsigned long long)stats.pixels_processed);
  std::fprintf(stderr, "  Total samples:         %llu\n", (unsigned long long)stats.samples_processed);
  std::fprintf(stderr, "  Total rays:            %llu\n", (unsigned long long)stats.rays_processed);
  std::fprintf(stderr, "  Total reflections:     %llu\n", (unsigned long long)stats.reflections);
  std::fprintf(stderr, "  Pixels per second:     %.2f pixels/s\n", double(stats.pixels_processed) / runtime);
  std::fprintf(stderr, "  Total runtime:         %.2f seconds\n", runtime);
  std::fprintf(stderr, "    Prepare runtime:     %.2f seconds\n", runtime - render_runtime);
  std::fprintf(stderr, "    Render runtime:      %.2f seconds\n", render_runtime);
  std::fprintf(stderr, "  Mrays/s (render):      %.2f  (zrt_render call %.2f s, %u GPU)\n",
               double(stats.rays_processed) / render_runtime / 1e6, call, stats.n_gpus);

  if (dn_env)
    std::fprintf(stderr, "  Denoise:               %u iterations, %.3f ms%s\n",
                 dn.iterations ? dn.iterations : unsigned(ZRT_DEFAULT_DENOISE_ITERATIONS), denoise_ms,
                 !var_env ? "" : dn_flags ? " (variance-guided, demodulated)" : " (variance-guided)");

  if (tf_env)
    std::fprintf(stderr, "  Temporal:              %u frames (the counters above are the last frame's)\n",
                 unsigned(cameras.size()));

  rc = zrt_image_write_png(filename, image.data(), width, height);
  if (const char* path = std::getenv("ZRT_DENOISE_NOISY"); path && dn_env && rc == ZRT_OK)
    rc = zrt_image_write_png(path, noisy.data(), width, height);
  if (const char* map = std::getenv("ZRT_ADAPTIVE_MAP"); map && tol_env && !dn_env && rc == ZRT_OK) {
    std::vector<float> grey(size_t(width) * height * 3);
    for (size_t i = 0; i < sample_map.size(); ++i)
      grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = float(sample_map[i]) / float(samples);
    rc = zrt_image_write_png(map, grey.data(), width, height);
  }
  // $ZRT_AO_OUT: the frame's AO plane as a grey PNG (zrt_render_ao, a launch of its own on the
  // first GPU); the frame above is what it was without it
  if (ao_out && rc == ZRT_OK) {
    std::vector<float> plane(size_t(width) * height), grey(size_t(width) * height * 3);
    rc = zrt_render_ao(scene, &camera, &ao_params, &ao, plane.data(), nullptr, nullptr);
    for (size_t i = 0; i < plane.size(); ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = plane[i];
    if (rc == ZRT_OK) rc = zrt_image_write_png(ao_out, grey.data(), width, height);
    if (rc == ZRT_OK) std::fprintf(stderr, "  Ambient occlusion:     %u rays per pixel -> %s\n", ao.n_samples, ao_out);
  }
  // $ZRT_PANORAMA_OUT: what the scene camera's origin sees in every direction (zrt_radiance, a
  // launch of its own on the first GPU); the frame above is what it was without it
  if (pano_out && rc == ZRT_OK) {
    const uint32_t pano_h = pano_w / 2, n = pano_w * pano_h;
    std::vector<float> rays(size_t(n) * 6), pano(size_t(n) * 3);
    const float origin[3] = {camera.origin.x, camera.origin.y, camera.origin.z};
    rc = zrt_rays_equirect(origin, pano_w, pano_h, rays.data());
    zrt_radiance_info info;
    if (rc == ZRT_OK) rc = zrt_radiance(scene, &ao_params, &pano_rq, rays.data(), n, nullptr, pano.data(), &info);
    if (rc == ZRT_OK) rc = zrt_image_write_png(pano_out, pano.data(), pano_w, pano_h);
    if (rc == ZRT_OK)
      std::fprintf(stderr, "  Panorama:              %ux%u, %u samples per ray, %llu rays -> %s\n", pano_w, pano_h,
                   pano_rq.n_samples, (unsigned long long)info.rays, pano_out);
  }
  // $ZRT_LENS_OUT: the frame through the lens at the scene camera's pose (zrt_render_lens, a launch
  // of its own on the first GPU); the frame above is what it was without it
  if (lens_out && rc == ZRT_OK) {
    std::vector<float> frame(size_t(width) * height * 3);
    zrt_radiance_info info;
    if (lens_dn)
      rc = zrt_render_lens_denoised(scene, &ao_params, &lens, &lens_q, nullptr, lens_dn_mode > 0 ? 1u : 0u,
                                    lens_dn_mode == 2 ? uint32_t(ZRT_DN_DEMODULATE) : 0u, frame.data(), nullptr, nullptr,
                                    nullptr, &info, nullptr);
    else
      rc = zrt_render_lens(scene, &ao_params, &lens, &lens_q, nullptr, frame.data(), &info);
    if (rc == ZRT_OK) rc = zrt_image_write_png(lens_out, frame.data(), width, height);
    if (rc == ZRT_OK)
      std::fprintf(stderr, "  Lens frame:            %s, %ux%u, %u samples per pixel, %llu rays -> %s\n", lens_name,
                   unsigned(width), unsigned(height), lens_q.n_samples, (unsigned long long)info.rays, lens_out);
    if (rc == ZRT_OK && lens_dn) std::fprintf(stderr, "  Lens frame filter:     %s\n", lens_dn);
  }
  zrt_scene_free(data);
  if (rc != ZRT_OK) {
    std::fprintf(stderr, "error: %s\n", zrt_last_error());
    return 1;
  }
  return 0;
}
