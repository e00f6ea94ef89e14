// y4m.hpp — the source side of the transcode job: raw 4:2:0 frames in YUV4MPEG2 framing.  The reference hands its FFmpeg child a
// container (`-i <file>`, internal/ffmpeg/transcode.go:68) that the child demuxes and decodes itself; this backend takes what such a
// decoder emits, from a FILE or from a STREAM: "-" / "pipe:0" (stdin) or a FIFO, so that any decoder process can feed it
// (`ffmpeg -i movie.mkv -f yuv4mpegpipe - | av1mi_transcode -i - ... out.mkv`).
//
// The encoder codes S closed GOPs of G frames in lockstep, i.e. it needs frames g*G + t of S different GOPs at the same time.  A
// seekable file with fixed-size frame headers is read in place (pread, one thread per segment).  Anything else is read
// sequentially, one GROUP of S*G frames ahead of the encoder, into host memory (two group buffers: S*G frames each).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace av1mi_host {

class Y4mSource {
 public:
  ~Y4mSource();
  int w = 0, h = 0, bd = 8, fps_n = 30, fps_d = 1;
  int sar_n = 1, sar_d = 1;      // the header's A<n>:<d> (sample aspect ratio); absent, A0:0 or malformed = 1:1
  int colour_range = -1;         // the header's XCOLORRANGE=FULL (1) | LIMITED (0); absent = -1; anything else is refused
  int interlace = 0;             // the header's I<c>: 0 progressive (Ip, I? or absent), 1 top field first (It), 2 bottom field first (Ib), 3 mixed (Im)
  // the source's own layout and depth (include/av1mi.h enum av1mi_source_chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4, 3 grey; 8, 10 or 12 bits);
  // bd above is the depth it is CODED at (12 -> 10).  Other than 4:2:0 at bd only after open(.., .., true)
  int chroma = 0, src_bd = 8;
  // false + *err (FFmpeg-style text) on a missing file, a header that is not Y4M, an unsupported colourspace or size.
  // any_layout: the job converts to 4:2:0 (a format= filter naming a 4:2:0 format, or -av1mi_format 420): C422, C444, Cmono and their
  // p10 / p12 (mono10 / mono12) forms and C420p12 are accepted besides C420* and C420p10; read() then delivers the source's layout
  bool open(const std::string &path, std::string *err, bool any_layout = false);
  bool seekable() const { return seekable_; }
  long known_frames() const { return seekable_ ? nframes_ : -1; }      // -1: a stream, the end is found by reading
  size_t frame_bytes() const { return frame_bytes_; }                  // one frame's samples in the file
  // the group of up to max_frames frames that starts at frame `first` (groups must be asked for in order, without gaps): returns how
  // many of them exist (0 = end of input), -1 on a malformed / truncated frame (*err)
  long prepare(long first, long max_frames, std::string *err);
  // frame i of the prepared group -> the three planes of the CODED size cw x ch (the true size rounded up to 8: the last column / row
  // replicated into the padding).  A source in another layout: its planes at the buffer sizes of that layout (av1mi.h "chroma formats":
  // 4:2:2 cw / 2 x ch, 4:4:4 cw x ch, grey none — U and V are not touched), uint16 samples for 10 and 12 bits.  Thread-safe for distinct
  // destinations.
  bool read(long i, int cw, int ch, unsigned char *Y, unsigned char *U, unsigned char *V) const;
  void close();

 private:
  FILE *f_ = nullptr;
  bool own_ = false, seekable_ = false;
  std::string path_;
  long hdr_len_ = 0, nframes_ = 0, group_first_ = 0;
  size_t frame_bytes_ = 0;
  // sequential mode: the current group and the one being read ahead
  std::vector<unsigned char> cur_, next_;
  long cur_n_ = 0, next_n_ = 0, next_first_ = 0;
  bool next_bad_ = false, eof_ = false;
  std::thread reader_;
  bool reader_running_ = false;
  void start_read_ahead(long first, long max_frames);
  long read_group(std::vector<unsigned char> &buf, long max_frames, bool *bad);
};

}  // namespace av1mi_host
