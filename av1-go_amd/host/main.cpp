// av1mi_transcode — CLI with the reference's process contract (exit code, stderr text, output file last):
//   av1mi_transcode [ffmpeg-style args] -i in.y4m [-global_quality:v:0 Q] [-g GOP] [-vf:v:0 CHAIN] [-av1mi_scale WxH]
//                   [-av1mi_stats FILE] [-av1mi_min_psnr DB] [-av1mi_me_range N] [-av1mi_format 420]
//                   [-b:v:0 BITS[k|M] | -av1mi_target_bpp X] [-qmin Q] [-qmax Q] out.av1-tmp.mkv
//                   (-b:v:0 / -av1mi_target_bpp: a target instead of the fixed quantiser; -global_quality is then where the controller starts)
//                   (-av1mi_format 420, or a format= filter naming a 4:2:0 format in CHAIN: 4:2:2 / 4:4:4 / grey and 12-bit sources are
//                   accepted and converted to 4:2:0 on the GPU)
//                   (-av1mi_stats: per-frame PSNR / SSIM measured on the GPU; -av1mi_min_psnr: fail with exit code 3 below that luma PSNR)
//                   (-av1mi_lr_search 0 | 1: 1 = a Wiener restoration record or none chosen per 64x64 unit on the GPU; the stats file's frame
//                   lines gain " lr:<units filtered>/<units>")
//                   (-av1mi_cdef_search 0 .. 3: N > 0 = one of 1 << N CDEF strength sets chosen per 64x64 superblock on the GPU, cdef_bits = N;
//                   the stats file's frame lines gain " cdef:<superblocks not on set 0>/<superblocks>")
//                   (-av1mi_lf_search 0 | 1: 1 = the deblocking levels of every frame chosen among 8 candidates on the GPU against the source;
//                   the stats file's frame lines gain " lf:<luma vertical level>/<chroma level>")
//                   (-av1mi_me_range: 0, or a multiple of 4 up to 64: the P frames' motion search follows N + 8 samples per frame)
//                   (CHAIN: the reference's scale filters, evaluated on the source's size and sample aspect ratio and applied on the GPU;
//                   -av1mi_scale: an explicit output size, wins over the chain; any other filter is refused)
//   av1mi_transcode --job in.y4m [--ratio 0.9] [--state DIR] [--wait S] [--replace-source 1] [--min-psnr DB] [--me-range N] [--format 420] [--target-bpp X]   (the ProcessJob lifecycle;
//                   the source is only replaced on request: the output is video-only)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include "daemon.hpp"

using namespace av1mi_host;

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "--gpu-usage")) {     // the AMD twin of internal/tui/gpu.go getGPUUsage
    printf("%.1f\n", GetGPUUsage(argc >= 3 ? atoi(argv[2]) : 0));
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "--job")) {
    Job job; job.ID = "cli"; job.SourcePath = argv[2];
    TranscodeConfig cfg; cfg.StableWaitSeconds = 0;
    for (int i = 3; i + 1 < argc; i += 2) {
      if (!strcmp(argv[i], "--ratio")) cfg.MaxSizeRatio = atof(argv[i + 1]);
      else if (!strcmp(argv[i], "--state")) cfg.JobStateDir = argv[i + 1];
      else if (!strcmp(argv[i], "--wait")) cfg.StableWaitSeconds = atoi(argv[i + 1]);
      else if (!strcmp(argv[i], "--replace-source")) { cfg.ReplaceSource = atoi(argv[i + 1]) != 0; }
      else if (!strcmp(argv[i], "--min-psnr")) cfg.MinPSNR = atof(argv[i + 1]);
      else if (!strcmp(argv[i], "--me-range")) cfg.MeRange = atoi(argv[i + 1]);
      else if (!strcmp(argv[i], "--format")) cfg.Format420 = !strcmp(argv[i + 1], "420");
      else if (!strcmp(argv[i], "--depth")) cfg.Depth = argv[i + 1];
      else if (!strcmp(argv[i], "--dither")) cfg.Dither = argv[i + 1];
      else if (!strcmp(argv[i], "--target-bpp")) cfg.TargetBitsPerPixel = atof(argv[i + 1]);
    }
    struct stat st;
    if (!stat(job.SourcePath.c_str(), &st)) job.OriginalSize = st.st_size;
    ProbeResult pr; pr.HasVideo = true; pr.has_video_stream = true; pr.VideoStream.Height = 1080;
    const std::string e = ProcessJob(&job, "av1mi", pr, cfg);
    fprintf(stderr, "job %s: %s%s%s\n", job.Status.c_str(), job.Reason.c_str(), e.empty() ? "" : " | ", e.c_str());
    return e.empty() ? 0 : 1;
  }
  if (argc >= 3 && !strcmp(argv[1], "--jobs")) {   // --jobs a.y4m b.y4m ... [--gpus N] [--workers W] [--ratio R] [--state DIR] [--min-psnr DB] [--me-range N] [--format 420]
    std::vector<Job> jobs;
    TranscodeConfig cfg; cfg.StableWaitSeconds = 0;
    int gpus = 1, workers = 0;
    for (int i = 2; i < argc; i++) {
      if (!strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--workers") && i + 1 < argc) workers = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--ratio") && i + 1 < argc) cfg.MaxSizeRatio = atof(argv[++i]);
      else if (!strcmp(argv[i], "--state") && i + 1 < argc) cfg.JobStateDir = argv[++i];
      else if (!strcmp(argv[i], "--min-psnr") && i + 1 < argc) cfg.MinPSNR = atof(argv[++i]);
      else if (!strcmp(argv[i], "--me-range") && i + 1 < argc) cfg.MeRange = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--format") && i + 1 < argc) cfg.Format420 = !strcmp(argv[++i], "420");
      else if (!strcmp(argv[i], "--depth") && i + 1 < argc) cfg.Depth = argv[++i];
      else if (!strcmp(argv[i], "--dither") && i + 1 < argc) cfg.Dither = argv[++i];
      else if (!strcmp(argv[i], "--target-bpp") && i + 1 < argc) cfg.TargetBitsPerPixel = atof(argv[++i]);
      else {
        Job j; j.ID = "job" + std::to_string(jobs.size()); j.SourcePath = argv[i];
        struct stat st;
        if (!stat(argv[i], &st)) j.OriginalSize = st.st_size;
        jobs.push_back(j);
      }
    }
    ProbeResult pr; pr.HasVideo = true; pr.has_video_stream = true; pr.VideoStream.Height = 1080;
    std::vector<std::string> errs;
    const PoolStats ps = RunJobPool(&jobs, workers > 0 ? workers : gpus, gpus, pr, cfg, &errs);
    for (size_t i = 0; i < jobs.size(); i++)
      fprintf(stderr, "%s %s: %s%s%s\n", jobs[i].ID.c_str(), jobs[i].Status.c_str(), jobs[i].Reason.c_str(), errs[i].empty() ? "" : " | ", errs[i].c_str());
    fprintf(stderr, "%d succeeded, %d skipped, %d failed in %.2f s\n", ps.succeeded, ps.skipped, ps.failed, ps.seconds);
    return ps.failed ? 1 : 0;
  }
  std::vector<std::string> args(argv + 1, argv + argc);
  const RunResult rr = RunTranscode(argv[0], args);
  if (rr.exitCode != 0) fprintf(stderr, "%s\n", rr.err.c_str());
  return rr.exitCode < 0 ? 255 : rr.exitCode;
}
