// vdf.hpp -- C++ host mirror of the reference crate's public surface for the hot path, over the C ABI
// (include/vdf.h).  Header-only; link with libvdf_hip.so.
//
// The reference is Rust and this image has no Rust toolchain, so this is the compiled-language host side above
// the boundary: same names, argument meaning and error behaviour as
//   vid_dup_finder_lib/src/lib.rs:132-140            VideoHash, MatchGroup, search, search_with_references, Error
//   vid_dup_finder_lib/src/video_hashing/video_hash.rs:26-32,45-73,176-192
//   vid_dup_finder_lib/src/video_hashing/video_dup_finder.rs:7-46
//   vid_dup_finder_lib/src/video_hashing/matches/match_group.rs:10-105
// What stays on the host (it needs paths): Search::sort (search_algorithm.rs:55-61) including Rust's
// component-wise PathBuf ordering; MatchGroup assembly from the index lists the library returns.
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/vdf.h"

namespace vdf {

// ---- Error (video_hashing/mod.rs:17-28) -------------------------------------------------------------------
struct Error : std::runtime_error {
    enum Kind { NotVideo, VidProc, NotEnoughFrames, Device } kind;
    Error(Kind k, const std::string &m) : std::runtime_error(m), kind(k) {}
    static Error not_enough_frames() { return Error(NotEnoughFrames, "Could not extract enough frames"); }
    static Error vid_proc(const std::string &m) { return Error(VidProc, "Video processing error: " + m); }
};
struct TooFewEntries : std::runtime_error {  // match_group.rs:15-16
    TooFewEntries() : std::runtime_error("too few entries") {}
};

// ---- a context: one GPU, or ONE context over several GPUs of the node ---------------------------------------
class Context {
public:
    explicit Context(int device = 0)
    {
        vdf_ctx *c = nullptr;
        if (vdf_ctx_create(device, &c) != VDF_OK) throw Error(Error::Device, vdf_last_error(nullptr));
        ctx_.reset(c, vdf_ctx_destroy);
    }
    // search() / search_with_references() / hashing then use every listed GPU from the one call (vdf_ctx_create_multi)
    explicit Context(const std::vector<int> &devices)
    {
        vdf_ctx *c = nullptr;
        if (vdf_ctx_create_multi(devices.data(), (int)devices.size(), &c) != VDF_OK) throw Error(Error::Device, vdf_last_error(nullptr));
        ctx_.reset(c, vdf_ctx_destroy);
    }
    int device_count() const { return vdf_ctx_device_count(ctx_.get()); }
    vdf_ctx *get() const { return ctx_.get(); }
    // VDF_DEVICES="0,1,2,3": the default context spans those GPUs (one process, vdf_ctx_create_multi); default: device 0
    static Context &default_context()
    {
        static Context c = [] {
            std::vector<int> devs;
            if (const char *e = std::getenv("VDF_DEVICES")) {
                const char *p = e;
                while (*p) {
                    char *end = nullptr;
                    const long v = std::strtol(p, &end, 10);
                    if (end == p) break;
                    devs.push_back((int)v);
                    p = (*end == ',') ? end + 1 : end;
                }
            }
            return devs.empty() ? Context(0) : Context(devs);
        }();
        return c;
    }

private:
    std::shared_ptr<vdf_ctx> ctx_;
};

// ---- Rust `PathBuf: Ord`: std::path compares Components, not bytes ------------------------------------------
// RootDir < CurDir < ParentDir < Normal(bytes); repeated '/' and inner "." are not components.
struct PathKey {
    std::vector<std::pair<int, std::string>> comps;
    explicit PathKey(const std::string &p)
    {
        if (!p.empty() && p[0] == '/') comps.emplace_back(1, "");
        else if (p == "." || p.rfind("./", 0) == 0) comps.emplace_back(2, "");
        size_t i = 0;
        while (i <= p.size()) {
            size_t j = p.find('/', i);
            if (j == std::string::npos) j = p.size();
            const std::string part = p.substr(i, j - i);
            if (!part.empty() && part != ".") comps.emplace_back(part == ".." ? 3 : 4, part == ".." ? "" : part);
            i = j + 1;
        }
    }
    bool operator<(const PathKey &o) const { return comps < o.comps; }
    bool operator==(const PathKey &o) const { return comps == o.comps; }
};

// ---- Crop (vid_dup_finder_common/src/crop.rs:3-10) ---------------------------------------------------------------
// The crop box of a frame as edge offsets: what the letterbox detection yields and crop_resize_buf takes; one row {left, right, top,
// bottom} of the C ABI's out_crops.  Member order = the derive's comparison order.
struct Crop {
    std::pair<uint32_t, uint32_t> orig_res{0, 0};
    uint32_t left = 0, right = 0, top = 0, bottom = 0;

    // crop.rs:13-30 (the reference asserts; a box that leaves no pixel throws here)
    static Crop from_edge_offsets(std::pair<uint32_t, uint32_t> res, uint32_t l, uint32_t r, uint32_t t, uint32_t b)
    {
        if ((uint64_t)l + r >= res.first || (uint64_t)t + b >= res.second) throw std::invalid_argument("crop box leaves no pixels");
        return Crop{res, l, r, t, b};
    }
    // crop.rs:32-50
    static Crop from_topleft_and_dims(std::pair<uint32_t, uint32_t> res, uint32_t x, uint32_t y, uint32_t w, uint32_t h)
    {
        if ((uint64_t)x + w > res.first || (uint64_t)y + h > res.second) throw std::invalid_argument("box outside the frame");
        return Crop{res, x, res.first - w - x, y, res.second - h - y};
    }
    static Crop from_abi(std::pair<uint32_t, uint32_t> res, const uint32_t *box) { return from_edge_offsets(res, box[0], box[1], box[2], box[3]); }
    // crop.rs:53-68: per-edge minimum (unites the crops of the probed frames)
    Crop unite(const Crop &o) const
    {
        return from_edge_offsets(orig_res, std::min(left, o.left), std::min(right, o.right), std::min(top, o.top), std::min(bottom, o.bottom));
    }
    // crop.rs:92-103: {x, y, width, height}
    std::array<uint32_t, 4> as_view_args() const
    {
        if ((uint64_t)left + right > orig_res.first || (uint64_t)top + bottom > orig_res.second) throw std::overflow_error("crop offsets exceed the frame");
        return {left, top, orig_res.first - (left + right), orig_res.second - (top + bottom)};
    }
    uint32_t width() const { return orig_res.first - (left + right); }
    uint32_t height() const { return orig_res.second - (top + bottom); }
    uint32_t area() const { return width() * height(); }
    bool is_uncropped() const { return left == 0 && right == 0 && top == 0 && bottom == 0; }
    bool operator==(const Crop &o) const { return orig_res == o.orig_res && left == o.left && right == o.right && top == o.top && bottom == o.bottom; }
    bool operator<(const Crop &o) const
    {
        return std::tie(orig_res, left, right, top, bottom) < std::tie(o.orig_res, o.left, o.right, o.top, o.bottom);
    }
};

// Which way a clip is flipped (not in the reference, which cannot see through a mirror: lib.rs:102-111): X = mirrored along the width,
// Y = flipped along the height, T = its 16 frames reversed; any combination - the `variant` of vdf_hash_variant.
enum Flip : uint32_t { FlipX = 1, FlipY = 2, FlipT = 4 };

// ---- VideoHash (video_hash.rs:26-32) ----------------------------------------------------------------------
class VideoHash {
public:
    using Words = std::array<uint64_t, VDF_HASH_WORDS>;
    VideoHash() : hash_{}, duration_(0) {}  // Default, video_hash.rs:34-42
    VideoHash(const std::array<uint64_t, VDF_HASH_WORDS> &h, std::string src_path, uint32_t duration)
        : hash_(h), src_path_(std::move(src_path)), duration_(duration) {}
    // ... with the clip's zero plane (bit i set iff DCT coefficient i is exactly 0.0): what flipped() needs.  The hash cache's wire format
    // has no room for it, so hashes loaded from a cache have none.  It takes no part in comparisons.
    VideoHash(const Words &h, std::string src_path, uint32_t duration, const Words &zero)
        : hash_(h), src_path_(std::move(src_path)), duration_(duration), zero_(zero) {}
    const std::optional<Words> &zero() const { return zero_; }

    // The VideoHash the same pipeline gives for the flipped clip (a combination of FlipX, FlipY, FlipT), from this hash and its zero plane
    // alone (vdf_hash_variant).  No zero plane -> Error::VidProc.
    VideoHash flipped(uint32_t flip) const
    {
        if (!zero_) throw Error::vid_proc("this VideoHash carries no zero plane (from_frame_stacks_planes; hashes loaded from a cache have none)");
        Words out{};
        if (vdf_hash_variant(hash_.data(), zero_->data(), flip, out.data()) != VDF_OK) throw std::invalid_argument("flip must be a combination of FlipX, FlipY, FlipT");
        return VideoHash(out, src_path_, duration_, *zero_);
    }

    // video_hash.rs:45-73.  frames: equal-size gray u8 frames (row-major, w x h); fewer than 16 (or none) ->
    // NotEnoughFrames; only the first 16 are used (dct_3d.rs:25).
    static VideoHash from_frames(const std::vector<const uint8_t *> &frames, uint32_t w, uint32_t h,
                                 const std::string &src_path, uint32_t duration, Context *ctx_opt = nullptr)
    {
        if (frames.size() < VDF_DCT_SIZE) throw Error::not_enough_frames();
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        std::vector<uint8_t> packed((size_t)VDF_DCT_SIZE * w * h);
        for (size_t f = 0; f < VDF_DCT_SIZE; f++) std::copy(frames[f], frames[f] + (size_t)w * h, packed.begin() + f * (size_t)w * h);
        std::array<uint64_t, VDF_HASH_WORDS> words{};
        const int rc = vdf_hash_frames_u8(ctx.get(), packed.data(), 1, VDF_DCT_SIZE, w, h, (size_t)w * h,
                                          (size_t)w * h * VDF_DCT_SIZE, words.data(), nullptr);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        return VideoHash(words, src_path, duration);
    }

    // The same for a batch of clips of DIFFERENT frame sizes in one call (vdf_hash_clips_u8): stack i = 16 tightly packed gray frames of
    // sizes[i] = (w, h).  One VideoHash per clip, in the caller's order.
    struct FrameStack {
        const uint8_t *frames;  // 16 x w x h bytes
        uint32_t w, h;
        std::string src_path;
        uint32_t duration;
    };
    static std::vector<VideoHash> from_frame_stacks(const std::vector<FrameStack> &stacks, Context *ctx_opt = nullptr)
    {
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        std::vector<vdf_clip> clips(stacks.size());
        size_t at = 0;
        for (size_t i = 0; i < stacks.size(); i++) {
            clips[i] = vdf_clip{at, (uint64_t)stacks[i].w * stacks[i].h, stacks[i].w, stacks[i].h, 0, 0, 0, 0};
            at += ((size_t)VDF_DCT_SIZE * stacks[i].w * stacks[i].h + 63) & ~(size_t)63;
        }
        std::vector<uint8_t> packed(at);
        for (size_t i = 0; i < stacks.size(); i++)
            std::copy(stacks[i].frames, stacks[i].frames + (size_t)VDF_DCT_SIZE * stacks[i].w * stacks[i].h, packed.begin() + (size_t)clips[i].offset);
        std::vector<uint64_t> words(stacks.size() * VDF_HASH_WORDS);
        const int rc = vdf_hash_clips_u8(ctx.get(), packed.data(), packed.size(), clips.data(), clips.size(), VDF_DCT_SIZE, words.data(), nullptr);
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<VideoHash> out;
        for (size_t i = 0; i < stacks.size(); i++) {
            std::array<uint64_t, VDF_HASH_WORDS> h;
            std::copy(words.begin() + i * VDF_HASH_WORDS, words.begin() + (i + 1) * VDF_HASH_WORDS, h.begin());
            out.emplace_back(h, stacks[i].src_path, stacks[i].duration);
        }
        return out;
    }

    // Every 16-frame window of every video (vdf_hash_windows_u8): frames = n_videos x frames_per_video tightly packed gray
    // frames of w x h.  Per video the VideoHash of frames [k * stride, k * stride + 16), k = 0 .. (frames_per_video - 16) / stride, each with
    // the video's path and duration: what finds a duplicate that is shifted in time.  Every frame is read and resized once.
    static std::vector<std::vector<VideoHash>> hash_windows(const uint8_t *frames, size_t n_videos, uint32_t frames_per_video, uint32_t w, uint32_t h,
                                                            uint32_t stride, const std::vector<std::string> &src_paths,
                                                            const std::vector<uint32_t> &durations, Context *ctx_opt = nullptr)
    {
        if (frames_per_video < VDF_DCT_SIZE) throw Error::not_enough_frames();
        if (src_paths.size() < n_videos || durations.size() < n_videos) throw std::invalid_argument("a path and a duration per video");
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const size_t n_win = vdf_hash_window_count(frames_per_video, stride), fs = (size_t)w * h;
        std::vector<uint64_t> words(n_videos * n_win * VDF_HASH_WORDS);
        const int rc = vdf_hash_windows_u8(ctx.get(), frames, n_videos, frames_per_video, w, h, fs, fs * frames_per_video, stride, words.data(), nullptr);
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<VideoHash>> out(n_videos);
        for (size_t i = 0; i < n_videos; i++)
            for (size_t k = 0; k < n_win; k++) {
                std::array<uint64_t, VDF_HASH_WORDS> hw;
                std::copy(words.begin() + (i * n_win + k) * VDF_HASH_WORDS, words.begin() + (i * n_win + k + 1) * VDF_HASH_WORDS, hw.begin());
                out[i].emplace_back(hw, src_paths[i], durations[i]);
            }
        return out;
    }
    // The same on device memory: d_out = n_clips x vdf_hash_window_count(frames_per_clip, stride) x 16 words, d_dontcare nullable.
    static void hash_windows_device(Context &ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                    size_t frame_stride, size_t clip_stride, uint32_t stride, uint64_t *d_out, uint32_t *d_dontcare = nullptr,
                                    void *stream = nullptr)
    {
        const int rc = vdf_hash_windows_u8_device(ctx.get(), d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, stride, d_out, d_dontcare, stream);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // Retimed windows (vdf_hash_windows_u8_retimed): hash_windows at rate_num / rate_den, 1 <= den <= num <= 2 den - window k =
    // the 16 frames k * stride + floor(i * num / den), which is what a copy at den / num of the frame rate (or sped up num / den) holds in its
    // plain windows.  Retime the side with more frames per second.
    static std::vector<std::vector<VideoHash>> hash_windows_retimed(const uint8_t *frames, size_t n_videos, uint32_t frames_per_video, uint32_t w, uint32_t h,
                                                                    uint32_t stride, uint32_t rate_num, uint32_t rate_den,
                                                                    const std::vector<std::string> &src_paths, const std::vector<uint32_t> &durations,
                                                                    Context *ctx_opt = nullptr)
    {
        if (src_paths.size() < n_videos || durations.size() < n_videos) throw std::invalid_argument("a path and a duration per video");
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const size_t n_win = vdf_hash_window_count_retimed(frames_per_video, stride, rate_num, rate_den), fs = (size_t)w * h;
        std::vector<uint64_t> words(n_videos * n_win * VDF_HASH_WORDS);
        const int rc = vdf_hash_windows_u8_retimed(ctx.get(), frames, n_videos, frames_per_video, w, h, fs, fs * frames_per_video, stride, rate_num, rate_den,
                                                   words.data(), nullptr);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<VideoHash>> out(n_videos);
        for (size_t i = 0; i < n_videos; i++)
            for (size_t k = 0; k < n_win; k++) {
                std::array<uint64_t, VDF_HASH_WORDS> hw;
                std::copy(words.begin() + (i * n_win + k) * VDF_HASH_WORDS, words.begin() + (i * n_win + k + 1) * VDF_HASH_WORDS, hw.begin());
                out[i].emplace_back(hw, src_paths[i], durations[i]);
            }
        return out;
    }
    // The same on device memory: d_out = n_clips x vdf_hash_window_count_retimed(frames_per_clip, stride, rate_num, rate_den) x 16 words.
    static void hash_windows_retimed_device(Context &ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                            size_t frame_stride, size_t clip_stride, uint32_t stride, uint32_t rate_num, uint32_t rate_den, uint64_t *d_out,
                                            uint32_t *d_dontcare = nullptr, void *stream = nullptr)
    {
        const int rc = vdf_hash_windows_u8_retimed_device(ctx.get(), d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, stride, rate_num,
                                                          rate_den, d_out, d_dontcare, stream);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // hash_windows_retimed at up to VDF_WINDOWS_MAX_RATES rates from ONE upload, one resize and one spatial transform of the frames
    // (vdf_hash_windows_u8_rates): out[r] = what hash_windows_retimed gives at rates[r] = {num, den}; {1, 1} gives the plain windows.
    static std::vector<std::vector<std::vector<VideoHash>>> hash_windows_rates(const uint8_t *frames, size_t n_videos, uint32_t frames_per_video, uint32_t w,
                                                                               uint32_t h, uint32_t stride, const std::vector<std::array<uint32_t, 2>> &rates,
                                                                               const std::vector<std::string> &src_paths,
                                                                               const std::vector<uint32_t> &durations, Context *ctx_opt = nullptr)
    {
        if (src_paths.size() < n_videos || durations.size() < n_videos) throw std::invalid_argument("a path and a duration per video");
        if (rates.empty() || rates.size() > VDF_WINDOWS_MAX_RATES) throw std::invalid_argument("1 ... 8 rates");
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const uint32_t n_rates = (uint32_t)rates.size();
        std::vector<uint32_t> num(n_rates), den(n_rates);
        for (uint32_t r = 0; r < n_rates; r++) { num[r] = rates[r][0]; den[r] = rates[r][1]; }
        std::vector<size_t> first(n_rates + 1);
        const size_t rows = vdf_hash_window_count_rates(n_videos, frames_per_video, stride, n_rates, num.data(), den.data(), first.data()), fs = (size_t)w * h;
        std::vector<uint64_t> words(rows * VDF_HASH_WORDS);
        const vdf_windows_rates_job job{frames, n_videos, frames_per_video, w, h, fs, fs * frames_per_video, stride, n_rates, num.data(), den.data(),
                                        words.data(), nullptr, nullptr};
        const int rc = vdf_hash_windows_u8_rates(ctx.get(), &job);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<std::vector<VideoHash>>> out(n_rates, std::vector<std::vector<VideoHash>>(n_videos));
        for (uint32_t r = 0; r < n_rates; r++) {
            const size_t n_win = n_videos ? (first[r + 1] - first[r]) / n_videos : 0;
            for (size_t i = 0; i < n_videos; i++)
                for (size_t k = 0; k < n_win; k++) {
                    const size_t row = first[r] + i * n_win + k;
                    std::array<uint64_t, VDF_HASH_WORDS> hw;
                    std::copy(words.begin() + row * VDF_HASH_WORDS, words.begin() + (row + 1) * VDF_HASH_WORDS, hw.begin());
                    out[r][i].emplace_back(hw, src_paths[i], durations[i]);
                }
        }
        return out;
    }
    // The same on device memory, ordered on `stream`: d_out = 16 words for each of vdf_hash_window_count_rates' rows, rate-major.
    static void hash_windows_rates_device(Context &ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                          size_t frame_stride, size_t clip_stride, uint32_t stride, const std::vector<std::array<uint32_t, 2>> &rates,
                                          uint64_t *d_out, uint32_t *d_dontcare = nullptr, void *stream = nullptr)
    {
        std::vector<uint32_t> num(rates.size()), den(rates.size());
        for (size_t r = 0; r < rates.size(); r++) { num[r] = rates[r][0]; den[r] = rates[r][1]; }
        const vdf_windows_rates_job job{d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, stride, (uint32_t)rates.size(), num.data(),
                                        den.data(), d_out, d_dontcare, stream};
        const int rc = vdf_hash_windows_u8_rates_device(ctx.get(), &job);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // Every window of videos of DIFFERENT frame sizes and lengths in one call (vdf_hash_windows_clips_u8): video i = n_frames
    // tightly packed gray frames of w x h, with an optional crop box {left, right, top, bottom} read in place.  Per video the VideoHash of
    // frames [k * stride, k * stride + 16); the lists differ in length.  The words are hash_windows' for each video alone.
    struct Video {
        const uint8_t *frames;  // n_frames x w x h bytes
        uint32_t n_frames, w, h;
        std::string src_path;
        uint32_t duration;
        std::array<uint32_t, 4> crop{{0, 0, 0, 0}};
    };
    static std::vector<std::vector<VideoHash>> hash_windows_clips(const std::vector<Video> &videos, uint32_t stride, Context *ctx_opt = nullptr)
    {
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const size_t n = videos.size();
        std::vector<vdf_clip> clips(n);
        std::vector<uint32_t> n_frames(n), first(n + 1);
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            const Video &v = videos[i];
            if (v.n_frames < VDF_DCT_SIZE) throw Error::not_enough_frames();
            clips[i] = vdf_clip{at, (uint64_t)v.w * v.h, v.w, v.h, v.crop[0], v.crop[1], v.crop[2], v.crop[3]};
            n_frames[i] = v.n_frames;
            at += ((size_t)v.n_frames * v.w * v.h + 63) & ~(size_t)63;
        }
        if (vdf_hash_windows_clips_first(n_frames.data(), n, stride, first.data()) != VDF_OK)
            throw std::invalid_argument("a window stride of zero, or 2^32 windows or more in one call");
        std::vector<uint8_t> packed(at);
        for (size_t i = 0; i < n; i++)
            std::copy(videos[i].frames, videos[i].frames + (size_t)videos[i].n_frames * videos[i].w * videos[i].h, packed.begin() + (size_t)clips[i].offset);
        std::vector<uint64_t> words((size_t)first[n] * VDF_HASH_WORDS);
        const int rc = vdf_hash_windows_clips_u8(ctx.get(), packed.data(), packed.size(), clips.data(), n_frames.data(), n, stride, words.data(), nullptr);
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<VideoHash>> out(n);
        for (size_t i = 0; i < n; i++)
            for (size_t r = first[i]; r < first[i + 1]; r++) {
                std::array<uint64_t, VDF_HASH_WORDS> hw;
                std::copy(words.begin() + r * VDF_HASH_WORDS, words.begin() + (r + 1) * VDF_HASH_WORDS, hw.begin());
                out[i].emplace_back(hw, videos[i].src_path, videos[i].duration);
            }
        return out;
    }
    // The same on device memory: clips and n_frames are HOST arrays (offsets relative to d_buf); d_out = first[n_videos] x 16 words with first
    // from vdf_hash_windows_clips_first, d_dontcare nullable; window k of video i at row first[i] + k.  Ordered on stream.
    static void hash_windows_clips_device(Context &ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                          uint32_t stride, uint64_t *d_out, uint32_t *d_dontcare = nullptr, void *stream = nullptr)
    {
        const int rc = vdf_hash_windows_clips_u8_device(ctx.get(), d_buf, buf_bytes, clips, n_frames, n_videos, stride, d_out, d_dontcare, stream);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // The RETIMED windows of videos of different frame sizes and lengths in one call (vdf_hash_windows_clips_u8_retimed):
    // hash_windows_clips' videos at hash_windows_retimed's rate.  Per video the VideoHash of its frames k * stride + floor(t * num / den) inside its
    // box; the words are hash_windows_retimed's for each video alone.  A video shorter than a window's span: not_enough_frames.
    static std::vector<std::vector<VideoHash>> hash_windows_clips_retimed(const std::vector<Video> &videos, uint32_t stride, uint32_t rate_num,
                                                                          uint32_t rate_den, Context *ctx_opt = nullptr)
    {
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const size_t n = videos.size();
        std::vector<vdf_clip> clips(n);
        std::vector<uint32_t> n_frames(n), first(n + 1);
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            const Video &v = videos[i];
            clips[i] = vdf_clip{at, (uint64_t)v.w * v.h, v.w, v.h, v.crop[0], v.crop[1], v.crop[2], v.crop[3]};
            n_frames[i] = v.n_frames;
            at += ((size_t)v.n_frames * v.w * v.h + 63) & ~(size_t)63;
        }
        const int rf = vdf_hash_windows_clips_first_retimed(n_frames.data(), n, stride, rate_num, rate_den, first.data());
        if (rf == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rf != VDF_OK) throw std::invalid_argument("a window stride of zero, a rate outside 1 <= den <= num <= 2 den, or 2^32 windows or more in one call");
        std::vector<uint8_t> packed(at);
        for (size_t i = 0; i < n; i++)
            std::copy(videos[i].frames, videos[i].frames + (size_t)videos[i].n_frames * videos[i].w * videos[i].h, packed.begin() + (size_t)clips[i].offset);
        std::vector<uint64_t> words((size_t)first[n] * VDF_HASH_WORDS);
        const int rc = vdf_hash_windows_clips_u8_retimed(ctx.get(), packed.data(), packed.size(), clips.data(), n_frames.data(), n, stride, rate_num, rate_den,
                                                         words.data(), nullptr);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<VideoHash>> out(n);
        for (size_t i = 0; i < n; i++)
            for (size_t r = first[i]; r < first[i + 1]; r++) {
                std::array<uint64_t, VDF_HASH_WORDS> hw;
                std::copy(words.begin() + r * VDF_HASH_WORDS, words.begin() + (r + 1) * VDF_HASH_WORDS, hw.begin());
                out[i].emplace_back(hw, videos[i].src_path, videos[i].duration);
            }
        return out;
    }
    // The same on device memory: clips and n_frames are HOST arrays; d_out = first[n_videos] x 16 words with first from
    // vdf_hash_windows_clips_first_retimed, d_dontcare nullable; retimed window k of video i at row first[i] + k.  Ordered on stream.
    static void hash_windows_clips_retimed_device(Context &ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                                  size_t n_videos, uint32_t stride, uint32_t rate_num, uint32_t rate_den, uint64_t *d_out,
                                                  uint32_t *d_dontcare = nullptr, void *stream = nullptr)
    {
        const int rc = vdf_hash_windows_clips_u8_retimed_device(ctx.get(), d_buf, buf_bytes, clips, n_frames, n_videos, stride, rate_num, rate_den, d_out,
                                                                d_dontcare, stream);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // hash_windows_clips_retimed at up to VDF_WINDOWS_MAX_RATES rates from ONE upload, one resize and one spatial transform of every frame
    // (vdf_hash_windows_clips_u8_rates): out[r] = what hash_windows_clips_retimed gives at rates[r] = {num, den}; {1, 1} gives the
    // plain windows.  A video shorter than the longest span of the list: not_enough_frames.
    static std::vector<std::vector<std::vector<VideoHash>>> hash_windows_clips_rates(const std::vector<Video> &videos, uint32_t stride,
                                                                                     const std::vector<std::array<uint32_t, 2>> &rates,
                                                                                     Context *ctx_opt = nullptr)
    {
        if (rates.empty() || rates.size() > VDF_WINDOWS_MAX_RATES) throw std::invalid_argument("1 ... 8 rates");
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const size_t n = videos.size();
        const uint32_t n_rates = (uint32_t)rates.size();
        std::vector<uint32_t> num(n_rates), den(n_rates);
        for (uint32_t r = 0; r < n_rates; r++) { num[r] = rates[r][0]; den[r] = rates[r][1]; }
        std::vector<vdf_clip> clips(n);
        std::vector<uint32_t> n_frames(n), first((size_t)n_rates * (n + 1));
        std::vector<size_t> rate_first(n_rates + 1);
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            const Video &v = videos[i];
            clips[i] = vdf_clip{at, (uint64_t)v.w * v.h, v.w, v.h, v.crop[0], v.crop[1], v.crop[2], v.crop[3]};
            n_frames[i] = v.n_frames;
            at += ((size_t)v.n_frames * v.w * v.h + 63) & ~(size_t)63;
        }
        const int rf = vdf_hash_windows_clips_first_rates(n_frames.data(), n, stride, n_rates, num.data(), den.data(), first.data(), rate_first.data());
        if (rf == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rf != VDF_OK) throw std::invalid_argument("a window stride of zero, a rate outside 1 <= den <= num <= 2 den, or 2^32 windows or more in one call");
        std::vector<uint8_t> packed(at);
        for (size_t i = 0; i < n; i++)
            std::copy(videos[i].frames, videos[i].frames + (size_t)videos[i].n_frames * videos[i].w * videos[i].h, packed.begin() + (size_t)clips[i].offset);
        std::vector<uint64_t> words(rate_first[n_rates] * VDF_HASH_WORDS);
        const vdf_windows_clips_rates_job job{packed.data(), packed.size(), clips.data(), n_frames.data(), n, stride, n_rates, num.data(), den.data(),
                                              words.data(), nullptr, nullptr};
        const int rc = vdf_hash_windows_clips_u8_rates(ctx.get(), &job);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<std::vector<VideoHash>>> out(n_rates, std::vector<std::vector<VideoHash>>(n));
        for (uint32_t r = 0; r < n_rates; r++)
            for (size_t i = 0; i < n; i++)
                for (size_t k = first[(size_t)r * (n + 1) + i]; k < first[(size_t)r * (n + 1) + i + 1]; k++) {
                    const size_t row = rate_first[r] + k;
                    std::array<uint64_t, VDF_HASH_WORDS> hw;
                    std::copy(words.begin() + row * VDF_HASH_WORDS, words.begin() + (row + 1) * VDF_HASH_WORDS, hw.begin());
                    out[r][i].emplace_back(hw, videos[i].src_path, videos[i].duration);
                }
        return out;
    }
    // The same on device memory, ordered on `stream`: clips and n_frames are HOST arrays; d_out = 16 words for each of
    // vdf_hash_windows_clips_first_rates' rows, rate-major: window k of video i at rate r at row rate_first[r] + first[r][i] + k.
    static void hash_windows_clips_rates_device(Context &ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                                size_t n_videos, uint32_t stride, const std::vector<std::array<uint32_t, 2>> &rates, uint64_t *d_out,
                                                uint32_t *d_dontcare = nullptr, void *stream = nullptr)
    {
        std::vector<uint32_t> num(rates.size()), den(rates.size());
        for (size_t r = 0; r < rates.size(); r++) { num[r] = rates[r][0]; den[r] = rates[r][1]; }
        const vdf_windows_clips_rates_job job{d_buf, buf_bytes, clips, n_frames, n_videos, stride, (uint32_t)rates.size(), num.data(), den.data(), d_out,
                                              d_dontcare, stream};
        const int rc = vdf_hash_windows_clips_u8_rates_device(ctx.get(), &job);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // Which videos share a stretch, at what offset, for how long (vdf_align_windows): windows_a / windows_b = hash_windows'
    // results (videos may differ in length); windows_b null: the videos of windows_a against each other, every pair a < b once.  At most one
    // record per pair of videos, in (a, b) order: the best run of consecutive windows within tol_int on one diagonal (offset = kb - ka), of at
    // least min_run windows.  skip_a / skip_b (optional): one byte per window in the order of the lists, non-zero = the window abstains
    // (static stretches).  One call of the C ABI: at most 2^24 pairs of videos.  ctx_opt null and a tiny input: walked on the CPU
    // (vdf_align_windows_host, the definition in plain C++).
    static std::vector<vdf_alignment> align_windows(const std::vector<std::vector<VideoHash>> &windows_a, const std::vector<std::vector<VideoHash>> *windows_b,
                                                    uint32_t tol_int, uint32_t min_run = 1, const std::vector<uint8_t> *skip_a = nullptr,
                                                    const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        auto csr = [](const std::vector<std::vector<VideoHash>> &w, std::vector<uint64_t> &words, std::vector<uint32_t> &first) {
            first.assign(1, 0u);
            for (const auto &video : w) {
                for (const VideoHash &h : video) words.insert(words.end(), h.words().begin(), h.words().end());
                first.push_back((uint32_t)(words.size() / VDF_HASH_WORDS));
            }
            if (words.empty()) words.push_back(0);  // a non-null pointer for an empty side
        };
        std::vector<uint64_t> wa, wb;
        std::vector<uint32_t> fa, fb;
        csr(windows_a, wa, fa);
        if (windows_b) csr(*windows_b, wb, fb);
        if (skip_a && skip_a->size() != fa.back()) throw std::invalid_argument("one skip byte per window of A");
        if (windows_b && skip_b && skip_b->size() != fb.back()) throw std::invalid_argument("one skip byte per window of B");
        const uint8_t *ska = skip_a && !skip_a->empty() ? skip_a->data() : nullptr, *skb = windows_b && skip_b && !skip_b->empty() ? skip_b->data() : nullptr;
        const size_t n_a = windows_a.size(), n_b = windows_b ? windows_b->size() : 0;
        const uint64_t cells = (uint64_t)fa.back() * (windows_b ? fb.back() : fa.back());
        std::vector<vdf_alignment> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && cells <= (1u << 16))
                rc = vdf_align_windows_host(wa.data(), fa.data(), n_a, ska, windows_b ? wb.data() : nullptr, fb.data(), n_b, skb, tol_int, min_run, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows(ctx.get(), wa.data(), fa.data(), n_a, ska, windows_b ? wb.data() : nullptr, fb.data(), n_b, skb, tol_int, min_run, out.data(),
                                       out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK) throw std::invalid_argument("align_windows: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // EVERY stretch two videos share (vdf_align_windows_stretches): align_windows' arguments, plus max_stretches (1 ... 8) records
    // per pair and the guard in windows.  Records in (a, b, rank) order: rank 0 is align_windows' record, rank r the best run of the pair's
    // matrix with the rectangles of the ranks before it - their windows of a x their windows of b, each widened by guard - masked.  ctx_opt
    // null and a tiny input: walked on the CPU (vdf_align_windows_stretches_host).
    static std::vector<vdf_alignment_stretch> align_windows_stretches(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                      const std::vector<std::vector<VideoHash>> *windows_b, uint32_t tol_int, uint32_t min_run = 1,
                                                                      uint32_t max_stretches = 4, uint32_t guard = 15, const std::vector<uint8_t> *skip_a = nullptr,
                                                                      const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        auto csr = [](const std::vector<std::vector<VideoHash>> &w, std::vector<uint64_t> &words, std::vector<uint32_t> &first) {
            first.assign(1, 0u);
            for (const auto &video : w) {
                for (const VideoHash &h : video) words.insert(words.end(), h.words().begin(), h.words().end());
                first.push_back((uint32_t)(words.size() / VDF_HASH_WORDS));
            }
            if (words.empty()) words.push_back(0);  // a non-null pointer for an empty side
        };
        std::vector<uint64_t> wa, wb;
        std::vector<uint32_t> fa, fb;
        csr(windows_a, wa, fa);
        if (windows_b) csr(*windows_b, wb, fb);
        if (skip_a && skip_a->size() != fa.back()) throw std::invalid_argument("one skip byte per window of A");
        if (windows_b && skip_b && skip_b->size() != fb.back()) throw std::invalid_argument("one skip byte per window of B");
        const uint8_t *ska = skip_a && !skip_a->empty() ? skip_a->data() : nullptr, *skb = windows_b && skip_b && !skip_b->empty() ? skip_b->data() : nullptr;
        const size_t n_a = windows_a.size(), n_b = windows_b ? windows_b->size() : 0;
        const uint64_t cells = (uint64_t)fa.back() * (windows_b ? fb.back() : fa.back());
        std::vector<vdf_alignment_stretch> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && cells <= (1u << 16))
                rc = vdf_align_windows_stretches_host(wa.data(), fa.data(), n_a, ska, windows_b ? wb.data() : nullptr, fb.data(), n_b, skb, tol_int, min_run, max_stretches,
                                                      guard, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_stretches(ctx.get(), wa.data(), fa.data(), n_a, ska, windows_b ? wb.data() : nullptr, fb.data(), n_b, skb, tol_int, min_run,
                                                 max_stretches, guard, out.data(), out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_stretches: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, max_stretches outside 1 ... 8, "
                                            "a guard above 2^20, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // ---- a library is not walked pair by pair: seed the candidate pairs, align only those ----
    // The two sides of an align call as the C ABI takes them, from hash_windows' lists.
    struct AlignSides {
        std::vector<uint64_t> wa, wb;
        std::vector<uint32_t> fa, fb;
        const uint8_t *ska = nullptr, *skb = nullptr;
        size_t n_a = 0, n_b = 0;
        bool self = true;
        uint64_t cells = 0;
        const uint64_t *b_words() const { return self ? nullptr : wb.data(); }
        AlignSides(const std::vector<std::vector<VideoHash>> &windows_a, const std::vector<std::vector<VideoHash>> *windows_b, const std::vector<uint8_t> *skip_a,
                   const std::vector<uint8_t> *skip_b)
        {
            auto csr = [](const std::vector<std::vector<VideoHash>> &w, std::vector<uint64_t> &words, std::vector<uint32_t> &first) {
                first.assign(1, 0u);
                for (const auto &video : w) {
                    for (const VideoHash &h : video) words.insert(words.end(), h.words().begin(), h.words().end());
                    first.push_back((uint32_t)(words.size() / VDF_HASH_WORDS));
                }
                if (words.empty()) words.push_back(0);  // a non-null pointer for an empty side
            };
            self = windows_b == nullptr;
            csr(windows_a, wa, fa);
            if (windows_b) csr(*windows_b, wb, fb);
            if (skip_a && skip_a->size() != fa.back()) throw std::invalid_argument("one skip byte per window of A");
            if (windows_b && skip_b && skip_b->size() != fb.back()) throw std::invalid_argument("one skip byte per window of B");
            ska = skip_a && !skip_a->empty() ? skip_a->data() : nullptr;
            skb = windows_b && skip_b && !skip_b->empty() ? skip_b->data() : nullptr;
            n_a = windows_a.size();
            n_b = windows_b ? windows_b->size() : 0;
            cells = (uint64_t)fa.back() * (windows_b ? fb.back() : fa.back());
        }
    };

    // Which pairs of videos can share a stretch at all (vdf_align_seed_pairs): align_windows' arguments; the pairs (a, b), in (a, b) order, with a
    // window ka of a, ka a multiple of min_run, and a window of b within tol_int of each other, neither skipped.  Every pair align_windows has a
    // record for is among them.  ctx_opt null and a tiny input: walked on the CPU (vdf_align_seed_pairs_host).
    static std::vector<vdf_video_pair> align_seed_pairs(const std::vector<std::vector<VideoHash>> &windows_a, const std::vector<std::vector<VideoHash>> *windows_b,
                                                        uint32_t tol_int, uint32_t min_run = 1, const std::vector<uint8_t> *skip_a = nullptr,
                                                        const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        const AlignSides s(windows_a, windows_b, skip_a, skip_b);
        std::vector<vdf_video_pair> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells <= (1u << 16))
                rc = vdf_align_seed_pairs_host(s.wa.data(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.fb.data(), s.n_b, s.skb, tol_int, min_run, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_seed_pairs(ctx.get(), s.wa.data(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.fb.data(), s.n_b, s.skb, tol_int, min_run, out.data(), out.size(),
                                          &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK) throw std::invalid_argument("align_seed_pairs: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // align_windows on the listed pairs only (vdf_align_windows_pairs): pairs strictly increasing in (a, b), a < b when windows_b is null.  The
    // records are align_windows' for those pairs, field for field - with align_seed_pairs' list, all of them.
    static std::vector<vdf_alignment> align_windows_pairs(const std::vector<std::vector<VideoHash>> &windows_a, const std::vector<std::vector<VideoHash>> *windows_b,
                                                          const std::vector<vdf_video_pair> &pairs, uint32_t tol_int, uint32_t min_run = 1,
                                                          const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                          Context *ctx_opt = nullptr)
    {
        const AlignSides s(windows_a, windows_b, skip_a, skip_b);
        std::vector<vdf_alignment> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells <= (1u << 16))
                rc = vdf_align_windows_pairs_host(s.wa.data(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.fb.data(), s.n_b, s.skb, pairs.empty() ? nullptr : pairs.data(),
                                                  pairs.size(), tol_int, min_run, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_pairs(ctx.get(), s.wa.data(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.fb.data(), s.n_b, s.skb, pairs.empty() ? nullptr : pairs.data(),
                                             pairs.size(), tol_int, min_run, out.data(), out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_pairs: min_run of 0, a video of more than 2^20 windows, more than 2^24 listed pairs, a list that is not strictly "
                                            "increasing, names a video that does not exist or has a >= b in self mode, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // align_windows_stretches on the listed pairs only (vdf_align_windows_stretches_pairs).
    static std::vector<vdf_alignment_stretch> align_windows_stretches_pairs(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                            const std::vector<std::vector<VideoHash>> *windows_b,
                                                                            const std::vector<vdf_video_pair> &pairs, uint32_t tol_int, uint32_t min_run = 1,
                                                                            uint32_t max_stretches = 4, uint32_t guard = 15, const std::vector<uint8_t> *skip_a = nullptr,
                                                                            const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        const AlignSides s(windows_a, windows_b, skip_a, skip_b);
        std::vector<vdf_alignment_stretch> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells <= (1u << 16))
                rc = vdf_align_windows_stretches_pairs_host(s.wa.data(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.fb.data(), s.n_b, s.skb,
                                                            pairs.empty() ? nullptr : pairs.data(), pairs.size(), tol_int, min_run, max_stretches, guard, out.data(),
                                                            out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_stretches_pairs(ctx.get(), s.wa.data(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.fb.data(), s.n_b, s.skb,
                                                       pairs.empty() ? nullptr : pairs.data(), pairs.size(), tol_int, min_run, max_stretches, guard, out.data(), out.size(),
                                                       &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_stretches_pairs: min_run of 0, a video of more than 2^20 windows, more than 2^24 listed pairs, max_stretches "
                                            "outside 1 ... 8, a guard above 2^20, a bad pair list, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // ---- a copy at another frame rate or speed: retimed windows of A against plain windows of B, every phase in one call ----
    // Which video of A is a copy of which video of B at rate_num / rate_den of its frames, and where (vdf_align_windows_retimed): windows_a =
    // hash_windows_retimed' lists at stride 1, windows_b = hash_windows' at stride 1; 1 <= den <= num <= 2 den, num <= VDF_ALIGN_RETIMED_MAX_NUM in
    // lowest terms.  At most one record per pair, in (a, b) order: the run's first windows first_a, first_b - its m-th cell is
    // (first_a + num m, first_b + den m) - its sub-sampled windows and the sum of their distances.  There is no self mode.  ctx_opt null and
    // a tiny input: walked on the CPU (vdf_align_windows_retimed_host, the definition in plain C++).
    static std::vector<vdf_alignment_retimed> align_windows_retimed(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                    const std::vector<std::vector<VideoHash>> &windows_b, uint32_t rate_num, uint32_t rate_den,
                                                                    uint32_t tol_int, uint32_t min_run = 1, const std::vector<uint8_t> *skip_a = nullptr,
                                                                    const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        const AlignSides s(windows_a, &windows_b, skip_a, skip_b);
        std::vector<vdf_alignment_retimed> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells <= (1u << 16))
                rc = vdf_align_windows_retimed_host(s.wa.data(), s.fa.data(), s.n_a, s.ska, s.wb.data(), s.fb.data(), s.n_b, s.skb, tol_int, min_run, rate_num, rate_den,
                                                    out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_retimed(ctx.get(), s.wa.data(), s.fa.data(), s.n_a, s.ska, s.wb.data(), s.fb.data(), s.n_b, s.skb, tol_int, min_run, rate_num,
                                               rate_den, out.data(), out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_retimed: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, a rate outside "
                                            "1 <= den <= num <= 2 den or with num above 32 in lowest terms, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // align_windows_retimed on the listed pairs only (vdf_align_windows_retimed_pairs): pairs strictly increasing in (a, b).  The records are
    // align_windows_retimed's for those pairs, field for field.  A library against itself: the list of the pairs a != b.
    static std::vector<vdf_alignment_retimed> align_windows_retimed_pairs(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                          const std::vector<std::vector<VideoHash>> &windows_b,
                                                                          const std::vector<vdf_video_pair> &pairs, uint32_t rate_num, uint32_t rate_den,
                                                                          uint32_t tol_int, uint32_t min_run = 1, const std::vector<uint8_t> *skip_a = nullptr,
                                                                          const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        const AlignSides s(windows_a, &windows_b, skip_a, skip_b);
        std::vector<vdf_alignment_retimed> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells <= (1u << 16))
                rc = vdf_align_windows_retimed_pairs_host(s.wa.data(), s.fa.data(), s.n_a, s.ska, s.wb.data(), s.fb.data(), s.n_b, s.skb,
                                                          pairs.empty() ? nullptr : pairs.data(), pairs.size(), tol_int, min_run, rate_num, rate_den, out.data(),
                                                          out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_retimed_pairs(ctx.get(), s.wa.data(), s.fa.data(), s.n_a, s.ska, s.wb.data(), s.fb.data(), s.n_b, s.skb,
                                                     pairs.empty() ? nullptr : pairs.data(), pairs.size(), tol_int, min_run, rate_num, rate_den, out.data(), out.size(),
                                                     &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_retimed_pairs: min_run of 0, a video of more than 2^20 windows, more than 2^24 listed pairs, a rate outside "
                                            "1 <= den <= num <= 2 den or with num above 32 in lowest terms, a bad pair list, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // The same on device memory (vdf_align_windows_retimed_device): d_* are device arrays as the C ABI takes them, the records come back to the host
    // and the call waits for its own work.
    static std::vector<vdf_alignment_retimed> align_windows_retimed_device(Context &ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                                                           const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                                                                           const uint8_t *d_b_skip, uint32_t rate_num, uint32_t rate_den, uint32_t tol_int,
                                                                           uint32_t min_run = 1, void *stream = nullptr)
    {
        std::vector<vdf_alignment_retimed> out(1024);
        for (;;) {
            size_t found = 0;
            const int rc = vdf_align_windows_retimed_device(ctx.get(), d_a_hashes, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip, tol_int, min_run,
                                                            rate_num, rate_den, out.data(), out.size(), &found, stream);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // ---- the retimed alignment seeded at every rate of a list, every phase, in one pass ----
    // Which pairs (a, b) can have a record of align_windows_retimed at which rate (vdf_align_seed_pairs_rates): windows_by_rate_a[r] =
    // hash_windows_retimed' lists of A at rates[r] (every rate over the same videos; what hash_windows_clips_rates returns), windows_b = plain windows
    // at stride 1; at most VDF_WINDOWS_MAX_RATES rates, duplicate and unreduced ones included.  The triples (a, b, rate index) in (rate, a, b) order:
    // the pairs with a window ka of a at that rate, (ka / num) % min_run == 0, and a window kb of b, kb % den == 0, within tol_int of each other,
    // neither skipped.  skip_a: one byte per window of A, rate-major (nullable); exclude_same: pairs (i, i) are never candidates.
    struct SeedRatesSides {
        std::vector<uint64_t> wa, wb;
        std::vector<uint32_t> fa, fb, num, den;  // fa: n_rates x (n_a + 1), every row counted from its block's first window
        std::vector<size_t> rate_first;
        size_t n_a = 0, n_b = 0;
        SeedRatesSides(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a, const std::vector<std::vector<VideoHash>> &windows_b,
                       const std::vector<std::pair<uint32_t, uint32_t>> &rates)
        {
            if (windows_by_rate_a.size() != rates.size()) throw std::invalid_argument("one set of windows of A per rate");
            n_a = rates.empty() ? 0 : windows_by_rate_a[0].size();
            n_b = windows_b.size();
            rate_first.assign(1, 0);
            for (size_t r = 0; r < rates.size(); r++) {
                if (windows_by_rate_a[r].size() != n_a) throw std::invalid_argument("every rate holds the windows of the same videos");
                num.push_back(rates[r].first);
                den.push_back(rates[r].second);
                uint32_t at = 0;
                fa.push_back(0u);
                for (const auto &video : windows_by_rate_a[r]) {
                    for (const VideoHash &h : video) wa.insert(wa.end(), h.words().begin(), h.words().end());
                    fa.push_back(at += (uint32_t)video.size());
                }
                rate_first.push_back(wa.size() / VDF_HASH_WORDS);
            }
            fb.assign(1, 0u);
            for (const auto &video : windows_b) {
                for (const VideoHash &h : video) wb.insert(wb.end(), h.words().begin(), h.words().end());
                fb.push_back((uint32_t)(wb.size() / VDF_HASH_WORDS));
            }
            if (wa.empty()) wa.push_back(0);  // a non-null pointer for an empty side
            if (wb.empty()) wb.push_back(0);
            if (fa.empty()) fa.push_back(0u);
        }
        vdf_align_seed_rates_job job(const std::vector<uint8_t> *skip_a, const std::vector<uint8_t> *skip_b, uint32_t tol_int, uint32_t min_run, bool exclude_same,
                                     std::vector<vdf_video_pair_rate> &out, size_t *found) const
        {
            if (skip_a && skip_a->size() != rate_first.back()) throw std::invalid_argument("one skip byte per window of A, rate-major");
            if (skip_b && skip_b->size() != fb.back()) throw std::invalid_argument("one skip byte per window of B");
            return vdf_align_seed_rates_job{wa.data(), fa.data(), rate_first.data(), skip_a && !skip_a->empty() ? skip_a->data() : nullptr, n_a, wb.data(), fb.data(),
                                            skip_b && !skip_b->empty() ? skip_b->data() : nullptr, n_b, (uint32_t)num.size(), num.empty() ? nullptr : num.data(),
                                            den.empty() ? nullptr : den.data(), tol_int, min_run, exclude_same ? 1u : 0u, out.data(), out.size(), found, nullptr};
        }
    };

    // the definition in plain C++ on the CPU (vdf_align_seed_pairs_rates_host): no context, no GPU
    static std::vector<vdf_video_pair_rate> align_seed_pairs_rates_host(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a,
                                                                        const std::vector<std::vector<VideoHash>> &windows_b,
                                                                        const std::vector<std::pair<uint32_t, uint32_t>> &rates, uint32_t tol_int,
                                                                        uint32_t min_run = 1, const std::vector<uint8_t> *skip_a = nullptr,
                                                                        const std::vector<uint8_t> *skip_b = nullptr, bool exclude_same = false)
    {
        const SeedRatesSides s(windows_by_rate_a, windows_b, rates);
        std::vector<vdf_video_pair_rate> out(1024);
        for (;;) {
            size_t found = 0;
            const vdf_align_seed_rates_job job = s.job(skip_a, skip_b, tol_int, min_run, exclude_same, out, &found);
            if (vdf_align_seed_pairs_rates_host(&job) != VDF_OK)
                throw std::invalid_argument("align_seed_pairs_rates: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, no or more than 8 rates, "
                                            "a rate outside 1 <= den <= num <= 2 den or with num above 32 in lowest terms, or exclude_same between sets of two sizes");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // one pass of the seed kernel over every phase of every rate (vdf_align_seed_pairs_rates): the host arrays go up once
    static std::vector<vdf_video_pair_rate> align_seed_pairs_rates(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a,
                                                                   const std::vector<std::vector<VideoHash>> &windows_b,
                                                                   const std::vector<std::pair<uint32_t, uint32_t>> &rates, uint32_t tol_int, uint32_t min_run = 1,
                                                                   const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                                   bool exclude_same = false, Context *ctx_opt = nullptr)
    {
        const SeedRatesSides s(windows_by_rate_a, windows_b, rates);
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        std::vector<vdf_video_pair_rate> out(1024);
        for (;;) {
            size_t found = 0;
            const vdf_align_seed_rates_job job = s.job(skip_a, skip_b, tol_int, min_run, exclude_same, out, &found);
            const int rc = vdf_align_seed_pairs_rates(ctx.get(), &job);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);
        }
    }

    // The same on device memory (vdf_align_seed_pairs_rates_device): the job's array pointers are device pointers - what
    // hash_windows_clips_rates_device wrote goes in unchanged - rate_num, rate_den and a_rate_first stay on the host; out, capacity and n_out of the
    // job are set here.  The triples come back to the host and the call waits for its own work on job.stream.
    static std::vector<vdf_video_pair_rate> align_seed_pairs_rates_device(Context &ctx, vdf_align_seed_rates_job job)
    {
        std::vector<vdf_video_pair_rate> out(1024);
        for (;;) {
            size_t found = 0;
            job.out = out.data(); job.capacity = out.size(); job.n_out = &found;
            const int rc = vdf_align_seed_pairs_rates_device(ctx.get(), &job);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // ---- the retimed alignment at every rate of a list in ONE call: (rate, a, b) triples ----
    // Which video of A is a copy of which video of B at which rate of the list, and where (vdf_align_windows_rates): the sides as
    // align_seed_pairs_rates takes them.  triples (nullable): only these, strictly increasing in (rate, a, b) - what align_seed_pairs_rates returned
    // goes in unchanged; null: every triple - without a == b under exclude_same - or, with seed, the candidates of the seed call, found inside the
    // call on arrays that went up once: the same records.  One vdf_alignment_rate per triple at most, in (rate, a, b) order.
    static vdf_align_rates_job align_rates_job(const SeedRatesSides &s, const std::vector<uint8_t> *skip_a, const std::vector<uint8_t> *skip_b, uint32_t tol_int,
                                               uint32_t min_run, const std::vector<vdf_video_pair_rate> *triples, bool seed, bool exclude_same,
                                               std::vector<vdf_alignment_rate> &out, size_t *found)
    {
        static const vdf_video_pair_rate no_triple{};  // an empty list must not read as "no list"
        std::vector<vdf_video_pair_rate> none;
        const vdf_align_seed_rates_job q = s.job(skip_a, skip_b, tol_int, min_run, exclude_same, none, found);
        return vdf_align_rates_job{q.a_hashes, q.a_first, q.a_rate_first, q.a_skip, q.n_a, q.b_hashes, q.b_first, q.b_skip, q.n_b, q.n_rates, q.rate_num, q.rate_den,
                                   tol_int, min_run, triples ? (triples->empty() ? &no_triple : triples->data()) : nullptr, triples ? triples->size() : 0,
                                   seed ? 1u : 0u, exclude_same ? 1u : 0u, out.data(), out.size(), found, nullptr};
    }

    // the definition in plain C++ on the CPU (vdf_align_windows_rates_host): no context, no GPU
    static std::vector<vdf_alignment_rate> align_windows_rates_host(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a,
                                                                    const std::vector<std::vector<VideoHash>> &windows_b,
                                                                    const std::vector<std::pair<uint32_t, uint32_t>> &rates, uint32_t tol_int, uint32_t min_run = 1,
                                                                    const std::vector<vdf_video_pair_rate> *triples = nullptr, bool seed = false,
                                                                    const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                                    bool exclude_same = false)
    {
        const SeedRatesSides s(windows_by_rate_a, windows_b, rates);
        std::vector<vdf_alignment_rate> out(1024);
        for (;;) {
            size_t found = 0;
            const vdf_align_rates_job job = align_rates_job(s, skip_a, skip_b, tol_int, min_run, triples, seed, exclude_same, out, &found);
            if (vdf_align_windows_rates_host(&job) != VDF_OK)
                throw std::invalid_argument("align_windows_rates: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, no or more than 8 rates, "
                                            "a rate outside 1 <= den <= num <= 2 den or with num above 32 in lowest terms, exclude_same between sets of two sizes, "
                                            "a list together with seed or exclude_same, or a list that is not strictly increasing in (rate, a, b) or names what is not there");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // through a context (vdf_align_windows_rates): the host arrays go up once, for the seed pass and the band walk alike
    static std::vector<vdf_alignment_rate> align_windows_rates(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a,
                                                               const std::vector<std::vector<VideoHash>> &windows_b,
                                                               const std::vector<std::pair<uint32_t, uint32_t>> &rates, uint32_t tol_int, uint32_t min_run = 1,
                                                               const std::vector<vdf_video_pair_rate> *triples = nullptr, bool seed = false,
                                                               const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                               bool exclude_same = false, Context *ctx_opt = nullptr)
    {
        const SeedRatesSides s(windows_by_rate_a, windows_b, rates);
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        std::vector<vdf_alignment_rate> out(1024);
        for (;;) {
            size_t found = 0;
            const vdf_align_rates_job job = align_rates_job(s, skip_a, skip_b, tol_int, min_run, triples, seed, exclude_same, out, &found);
            const int rc = vdf_align_windows_rates(ctx.get(), &job);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);
        }
    }

    // The same on device memory (vdf_align_windows_rates_device): the job's hashes, first arrays and skip bytes are device pointers - what
    // hash_windows_clips_rates_device wrote goes in unchanged - rate_num, rate_den, a_rate_first and triples stay on the host; out, capacity and n_out
    // of the job are set here.  The records come back to the host and the call waits for its own work on job.stream.
    static std::vector<vdf_alignment_rate> align_windows_rates_device(Context &ctx, vdf_align_rates_job job)
    {
        std::vector<vdf_alignment_rate> out(1024);
        for (;;) {
            size_t found = 0;
            job.out = out.data(); job.capacity = out.size(); job.n_out = &found;
            const int rc = vdf_align_windows_rates_device(ctx.get(), &job);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // ---- EVERY stretch of a retimed pair, ranked, at every rate of a list in one call ----
    // align_windows_rates with up to max_stretches (1 ... 8) records per triple (vdf_align_windows_rates_stretches): rank 0 is that call's record;
    // after every reported stretch its rectangle - in the rows of the two videos, widened by guard rows of b and ceil(guard num / den) of a -
    // counts as non-matching in EVERY phase, and the next rank is the best record of what is left.  Records in (rate, a, b, rank) order.
    static vdf_align_rates_stretches_job align_rates_stretches_job(const SeedRatesSides &s, const std::vector<uint8_t> *skip_a, const std::vector<uint8_t> *skip_b,
                                                                   uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard,
                                                                   const std::vector<vdf_video_pair_rate> *triples, bool seed, bool exclude_same,
                                                                   std::vector<vdf_alignment_rate_stretch> &out, size_t *found)
    {
        std::vector<vdf_alignment_rate> none;
        const vdf_align_rates_job q = align_rates_job(s, skip_a, skip_b, tol_int, min_run, triples, seed, exclude_same, none, found);
        return vdf_align_rates_stretches_job{q.a_hashes, q.a_first, q.a_rate_first, q.a_skip, q.n_a, q.b_hashes, q.b_first, q.b_skip, q.n_b, q.n_rates, q.rate_num,
                                             q.rate_den, tol_int, min_run, q.triples, q.n_triples, q.seed, q.exclude_same, max_stretches, guard, out.data(), out.size(),
                                             found, nullptr};
    }

    // the definition in plain C++ on the CPU (vdf_align_windows_rates_stretches_host): no context, no GPU
    static std::vector<vdf_alignment_rate_stretch> align_windows_rates_stretches_host(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a,
                                                                                     const std::vector<std::vector<VideoHash>> &windows_b,
                                                                                     const std::vector<std::pair<uint32_t, uint32_t>> &rates, uint32_t tol_int,
                                                                                     uint32_t min_run = 1, uint32_t max_stretches = 4, uint32_t guard = 15,
                                                                                     const std::vector<vdf_video_pair_rate> *triples = nullptr, bool seed = false,
                                                                                     const std::vector<uint8_t> *skip_a = nullptr,
                                                                                     const std::vector<uint8_t> *skip_b = nullptr, bool exclude_same = false)
    {
        const SeedRatesSides s(windows_by_rate_a, windows_b, rates);
        std::vector<vdf_alignment_rate_stretch> out(1024);
        for (;;) {
            size_t found = 0;
            const vdf_align_rates_stretches_job job = align_rates_stretches_job(s, skip_a, skip_b, tol_int, min_run, max_stretches, guard, triples, seed, exclude_same, out, &found);
            if (vdf_align_windows_rates_stretches_host(&job) != VDF_OK)
                throw std::invalid_argument("align_windows_rates_stretches: what align_windows_rates refuses, max_stretches outside 1 ... 8, or guard above 2^20");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // through a context (vdf_align_windows_rates_stretches): the host arrays go up once, for the seed pass and every round
    static std::vector<vdf_alignment_rate_stretch> align_windows_rates_stretches(const std::vector<std::vector<std::vector<VideoHash>>> &windows_by_rate_a,
                                                                                const std::vector<std::vector<VideoHash>> &windows_b,
                                                                                const std::vector<std::pair<uint32_t, uint32_t>> &rates, uint32_t tol_int,
                                                                                uint32_t min_run = 1, uint32_t max_stretches = 4, uint32_t guard = 15,
                                                                                const std::vector<vdf_video_pair_rate> *triples = nullptr, bool seed = false,
                                                                                const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                                                bool exclude_same = false, Context *ctx_opt = nullptr)
    {
        const SeedRatesSides s(windows_by_rate_a, windows_b, rates);
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        std::vector<vdf_alignment_rate_stretch> out(1024);
        for (;;) {
            size_t found = 0;
            const vdf_align_rates_stretches_job job = align_rates_stretches_job(s, skip_a, skip_b, tol_int, min_run, max_stretches, guard, triples, seed, exclude_same, out, &found);
            const int rc = vdf_align_windows_rates_stretches(ctx.get(), &job);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);
        }
    }

    // The same on device memory (vdf_align_windows_rates_stretches_device): the job's hashes, first arrays and skip bytes are device pointers; rate_num,
    // rate_den, a_rate_first and triples stay on the host; out, capacity and n_out of the job are set here.  The records come back to the host and
    // the call waits for its own work on job.stream.
    static std::vector<vdf_alignment_rate_stretch> align_windows_rates_stretches_device(Context &ctx, vdf_align_rates_stretches_job job)
    {
        std::vector<vdf_alignment_rate_stretch> out(1024);
        for (;;) {
            size_t found = 0;
            job.out = out.data(); job.capacity = out.size(); job.n_out = &found;
            const int rc = vdf_align_windows_rates_stretches_device(ctx.get(), &job);
            if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
            if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // hash_windows with the zero plane of every window (vdf_hash_windows_u8_planes): the same words, and every VideoHash
    // carries zero() - what align_windows_variants needs of the flipped side.
    static std::vector<std::vector<VideoHash>> hash_windows_planes(const uint8_t *frames, size_t n_videos, uint32_t frames_per_video, uint32_t w, uint32_t h,
                                                                   uint32_t stride, const std::vector<std::string> &src_paths,
                                                                   const std::vector<uint32_t> &durations, Context *ctx_opt = nullptr)
    {
        if (frames_per_video < VDF_DCT_SIZE) throw Error::not_enough_frames();
        if (src_paths.size() < n_videos || durations.size() < n_videos) throw std::invalid_argument("a path and a duration per video");
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        const size_t n_win = vdf_hash_window_count(frames_per_video, stride), fs = (size_t)w * h;
        std::vector<uint64_t> words(n_videos * n_win * VDF_HASH_WORDS), zero(words.size());
        const int rc = vdf_hash_windows_u8_planes(ctx.get(), frames, n_videos, frames_per_video, w, h, fs, fs * frames_per_video, stride, words.data(), nullptr,
                                                  zero.data());
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<std::vector<VideoHash>> out(n_videos);
        for (size_t i = 0; i < n_videos; i++)
            for (size_t k = 0; k < n_win; k++) {
                std::array<uint64_t, VDF_HASH_WORDS> hw, zw;
                std::copy(words.begin() + (i * n_win + k) * VDF_HASH_WORDS, words.begin() + (i * n_win + k + 1) * VDF_HASH_WORDS, hw.begin());
                std::copy(zero.begin() + (i * n_win + k) * VDF_HASH_WORDS, zero.begin() + (i * n_win + k + 1) * VDF_HASH_WORDS, zw.begin());
                out[i].emplace_back(hw, src_paths[i], durations[i], zw);
            }
        return out;
    }
    static void hash_windows_planes_device(Context &ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                           size_t frame_stride, size_t clip_stride, uint32_t stride, uint64_t *d_out, uint64_t *d_zero,
                                           uint32_t *d_dontcare = nullptr, void *stream = nullptr)
    {
        const int rc = vdf_hash_windows_u8_planes_device(ctx.get(), d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, stride, d_out, d_dontcare,
                                                         d_zero, stream);
        if (rc == VDF_E_NOT_ENOUGH_FRAMES) throw Error::not_enough_frames();
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }
    // The variant of a set of resident window hashes (vdf_window_variants_device): d_out (and d_out_skip, iff d_skip) = the set flipped by
    // `flip`, every video's rows in reversed order with FlipT.
    static void window_variants(Context &ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_first, size_t n_videos, uint32_t flip,
                                uint64_t *d_out, const uint8_t *d_skip = nullptr, uint8_t *d_out_skip = nullptr, void *stream = nullptr)
    {
        const int rc = vdf_window_variants_device(ctx.get(), d_hashes, d_zero, d_first, n_videos, d_skip, flip, d_out, d_out_skip, stream);
        if (rc == VDF_E_INVAL) throw std::invalid_argument(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    }

    // align_windows against the flipped videos of B (vdf_align_windows_variants): for every flip of `flips` (each 1 ... 7) the
    // records of align_windows on the window hashes of the flipped b, in (variant, a, b) order.  The hashes of the flipped side (windows_b, or
    // windows_a when windows_b is null) need their zero planes (hash_windows_planes), else Error::VidProc.  offset and start_a + offset count in
    // the DERIVED order of b: with FlipT derived window j is b's window Nb - 1 - j, and the stretch runs backwards through b.
    static std::vector<vdf_alignment_variant> align_windows_variants(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                     const std::vector<std::vector<VideoHash>> *windows_b, uint32_t tol_int,
                                                                     const std::vector<uint32_t> &flips, uint32_t min_run = 1,
                                                                     const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                                     Context *ctx_opt = nullptr)
    {
        auto csr = [](const std::vector<std::vector<VideoHash>> &w, std::vector<uint64_t> &words, std::vector<uint64_t> *zero, std::vector<uint32_t> &first) {
            first.assign(1, 0u);
            for (const auto &video : w) {
                for (const VideoHash &h : video) {
                    words.insert(words.end(), h.words().begin(), h.words().end());
                    if (zero) {
                        if (!h.zero()) throw Error::vid_proc("align_windows_variants needs the zero plane of every hash of the flipped side (hash_windows_planes)");
                        zero->insert(zero->end(), h.zero()->begin(), h.zero()->end());
                    }
                }
                first.push_back((uint32_t)(words.size() / VDF_HASH_WORDS));
            }
            if (words.empty()) words.push_back(0);  // a non-null pointer for an empty side
            if (zero && zero->empty()) zero->push_back(0);
        };
        uint32_t mask = 0;
        for (uint32_t f : flips) {
            if (f < 1 || f > 7) throw std::invalid_argument("flips are non-empty combinations of FlipX, FlipY, FlipT");
            mask |= 1u << f;
        }
        std::vector<uint64_t> wa, wb, za, zb;
        std::vector<uint32_t> fa, fb;
        csr(windows_a, wa, windows_b ? nullptr : &za, fa);
        if (windows_b) csr(*windows_b, wb, &zb, fb);
        if (skip_a && skip_a->size() != fa.back()) throw std::invalid_argument("one skip byte per window of A");
        if (windows_b && skip_b && skip_b->size() != fb.back()) throw std::invalid_argument("one skip byte per window of B");
        const uint8_t *ska = skip_a && !skip_a->empty() ? skip_a->data() : nullptr, *skb = windows_b && skip_b && !skip_b->empty() ? skip_b->data() : nullptr;
        const size_t n_a = windows_a.size(), n_b = windows_b ? windows_b->size() : 0;
        const uint64_t cells = (uint64_t)fa.back() * (windows_b ? fb.back() : fa.back()) * flips.size();
        std::vector<vdf_alignment_variant> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && cells <= (1u << 16))
                rc = vdf_align_windows_variants_host(wa.data(), windows_b ? nullptr : za.data(), fa.data(), n_a, ska, windows_b ? wb.data() : nullptr,
                                                     windows_b ? zb.data() : nullptr, fb.data(), n_b, skb, tol_int, min_run, mask, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_variants(ctx.get(), wa.data(), windows_b ? nullptr : za.data(), fa.data(), n_a, ska, windows_b ? wb.data() : nullptr,
                                                windows_b ? zb.data() : nullptr, fb.data(), n_b, skb, tol_int, min_run, mask, out.data(), out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_variants: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // The arrays of the two calls below, as align_windows_variants builds its own: hashes, zero planes of the flipped side, first arrays, skip bytes.
    struct AlignVariantSides {
        std::vector<uint64_t> wa, wb, za, zb;
        std::vector<uint32_t> fa, fb;
        const uint8_t *ska = nullptr, *skb = nullptr;
        size_t n_a = 0, n_b = 0;
        bool two_sets = false;
        uint64_t cells = 0;
        AlignVariantSides(const char *what, const std::vector<std::vector<VideoHash>> &windows_a, const std::vector<std::vector<VideoHash>> *windows_b,
                          const std::vector<uint8_t> *skip_a, const std::vector<uint8_t> *skip_b)
        {
            auto csr = [what](const std::vector<std::vector<VideoHash>> &w, std::vector<uint64_t> &words, std::vector<uint64_t> *zero, std::vector<uint32_t> &first) {
                first.assign(1, 0u);
                for (const auto &video : w) {
                    for (const VideoHash &h : video) {
                        words.insert(words.end(), h.words().begin(), h.words().end());
                        if (zero) {
                            if (!h.zero()) throw Error::vid_proc(std::string(what) + " needs the zero plane of every hash of the flipped side (hash_windows_planes)");
                            zero->insert(zero->end(), h.zero()->begin(), h.zero()->end());
                        }
                    }
                    first.push_back((uint32_t)(words.size() / VDF_HASH_WORDS));
                }
                if (words.empty()) words.push_back(0);  // a non-null pointer for an empty side
                if (zero && zero->empty()) zero->push_back(0);
            };
            two_sets = windows_b != nullptr;
            csr(windows_a, wa, two_sets ? nullptr : &za, fa);
            if (two_sets) csr(*windows_b, wb, &zb, fb);
            if (skip_a && skip_a->size() != fa.back()) throw std::invalid_argument("one skip byte per window of A");
            if (two_sets && skip_b && skip_b->size() != fb.back()) throw std::invalid_argument("one skip byte per window of B");
            ska = skip_a && !skip_a->empty() ? skip_a->data() : nullptr;
            skb = two_sets && skip_b && !skip_b->empty() ? skip_b->data() : nullptr;
            n_a = windows_a.size();
            n_b = two_sets ? windows_b->size() : 0;
            cells = (uint64_t)fa.back() * (two_sets ? fb.back() : fa.back());
        }
        const uint64_t *a_zero() const { return two_sets ? nullptr : za.data(); }
        const uint64_t *b_words() const { return two_sets ? wb.data() : nullptr; }
        const uint64_t *b_zero() const { return two_sets ? zb.data() : nullptr; }
    };

    // Which pairs of videos can share a FLIPPED stretch at all (vdf_align_seed_pairs_variants): align_windows_variants' arguments;
    // the (variant, a, b) triples, in that order, that are candidates of align_seed_pairs on (A, the flipped B) - every triple
    // align_windows_variants has a record for is among them, and on a context all flips come from one pass over the seeds.
    static std::vector<vdf_video_pair_variant> align_seed_pairs_variants(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                         const std::vector<std::vector<VideoHash>> *windows_b, uint32_t tol_int,
                                                                         const std::vector<uint32_t> &flips, uint32_t min_run = 1,
                                                                         const std::vector<uint8_t> *skip_a = nullptr, const std::vector<uint8_t> *skip_b = nullptr,
                                                                         Context *ctx_opt = nullptr)
    {
        uint32_t mask = 0;
        for (uint32_t f : flips) {
            if (f < 1 || f > 7) throw std::invalid_argument("flips are non-empty combinations of FlipX, FlipY, FlipT");
            mask |= 1u << f;
        }
        const AlignVariantSides s("align_seed_pairs_variants", windows_a, windows_b, skip_a, skip_b);
        std::vector<vdf_video_pair_variant> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells * flips.size() <= (1u << 16))
                rc = vdf_align_seed_pairs_variants_host(s.wa.data(), s.a_zero(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.b_zero(), s.fb.data(), s.n_b, s.skb, tol_int,
                                                        min_run, mask, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_seed_pairs_variants(ctx.get(), s.wa.data(), s.a_zero(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.b_zero(), s.fb.data(), s.n_b, s.skb,
                                                   tol_int, min_run, mask, out.data(), out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_seed_pairs_variants: min_run of 0, a video of more than 2^20 windows, more than 2^24 pairs, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);  // the buffer was too small: once more with room for all
        }
    }

    // align_windows_variants on the listed (variant, a, b) triples only (vdf_align_windows_variants_pairs): strictly increasing in (variant, a, b),
    // every variant 1 ... 7, a < b when windows_b is null.  The records are align_windows_variants' for those triples, field for field - with
    // align_seed_pairs_variants' list, all of them.
    static std::vector<vdf_alignment_variant> align_windows_variants_pairs(const std::vector<std::vector<VideoHash>> &windows_a,
                                                                           const std::vector<std::vector<VideoHash>> *windows_b,
                                                                           const std::vector<vdf_video_pair_variant> &triples, uint32_t tol_int,
                                                                           uint32_t min_run = 1, const std::vector<uint8_t> *skip_a = nullptr,
                                                                           const std::vector<uint8_t> *skip_b = nullptr, Context *ctx_opt = nullptr)
    {
        const AlignVariantSides s("align_windows_variants_pairs", windows_a, windows_b, skip_a, skip_b);
        const vdf_video_pair_variant *list = triples.empty() ? nullptr : triples.data();
        std::vector<vdf_alignment_variant> out(1024);
        for (;;) {
            size_t found = 0;
            int rc;
            if (!ctx_opt && s.cells * 7 <= (1u << 16))
                rc = vdf_align_windows_variants_pairs_host(s.wa.data(), s.a_zero(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.b_zero(), s.fb.data(), s.n_b, s.skb, list,
                                                           triples.size(), tol_int, min_run, out.data(), out.size(), &found);
            else {
                Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
                rc = vdf_align_windows_variants_pairs(ctx.get(), s.wa.data(), s.a_zero(), s.fa.data(), s.n_a, s.ska, s.b_words(), s.b_zero(), s.fb.data(), s.n_b, s.skb,
                                                      list, triples.size(), tol_int, min_run, out.data(), out.size(), &found);
                if (rc != VDF_OK && rc != VDF_E_INVAL) throw Error(Error::Device, vdf_last_error(ctx.get()));
            }
            if (rc != VDF_OK)
                throw std::invalid_argument("align_windows_variants_pairs: a list that is not strictly increasing in (variant, a, b) or names a variant or a video that "
                                            "does not exist, min_run of 0, a video of more than 2^20 windows, more than 2^24 triples, or a multi-GPU context");
            if (found <= out.size()) { out.resize(found); return out; }
            out.resize(found);
        }
    }

    // from_frame_stacks with the zero planes (vdf_hash_clips_u8_planes): the hashes are the same words and can be flipped.  crops (optional, one
    // l, r, t, b per clip - e.g. what from_frame_stacks_letterbox detected): hash, plane and every flip are those of the CROPPED clip.
    static std::vector<VideoHash> from_frame_stacks_planes(const std::vector<FrameStack> &stacks, const std::vector<std::array<uint32_t, 4>> *crops = nullptr,
                                                           Context *ctx_opt = nullptr)
    {
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        if (crops && crops->size() != stacks.size()) throw std::invalid_argument("one crop box per clip");
        std::vector<vdf_clip> clips(stacks.size());
        size_t at = 0;
        for (size_t i = 0; i < stacks.size(); i++) {
            const std::array<uint32_t, 4> c = crops ? (*crops)[i] : std::array<uint32_t, 4>{0, 0, 0, 0};
            clips[i] = vdf_clip{at, (uint64_t)stacks[i].w * stacks[i].h, stacks[i].w, stacks[i].h, c[0], c[1], c[2], c[3]};
            at += ((size_t)VDF_DCT_SIZE * stacks[i].w * stacks[i].h + 63) & ~(size_t)63;
        }
        std::vector<uint8_t> packed(at);
        for (size_t i = 0; i < stacks.size(); i++)
            std::copy(stacks[i].frames, stacks[i].frames + (size_t)VDF_DCT_SIZE * stacks[i].w * stacks[i].h, packed.begin() + (size_t)clips[i].offset);
        std::vector<uint64_t> words(stacks.size() * VDF_HASH_WORDS), zero(stacks.size() * VDF_HASH_WORDS);
        const int rc = vdf_hash_clips_u8_planes(ctx.get(), packed.data(), packed.size(), clips.data(), clips.size(), VDF_DCT_SIZE, words.data(), nullptr, zero.data());
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<VideoHash> out;
        for (size_t i = 0; i < stacks.size(); i++) {
            Words h, z;
            std::copy(words.begin() + i * VDF_HASH_WORDS, words.begin() + (i + 1) * VDF_HASH_WORDS, h.begin());
            std::copy(zero.begin() + i * VDF_HASH_WORDS, zero.begin() + (i + 1) * VDF_HASH_WORDS, z.begin());
            out.emplace_back(h, stacks[i].src_path, stacks[i].duration, z);
        }
        return out;
    }

    // ... with Cropdetect::Letterbox first, the builder's default (vdf_hash_clips_u8_letterbox); crops_out (optional): l, r, t, b per clip
    static std::vector<VideoHash> from_frame_stacks_letterbox(const std::vector<FrameStack> &stacks, std::vector<std::array<uint32_t, 4>> *crops_out = nullptr,
                                                              Context *ctx_opt = nullptr)
    {
        Context &ctx = ctx_opt ? *ctx_opt : Context::default_context();
        std::vector<vdf_clip> clips(stacks.size());
        size_t at = 0;
        for (size_t i = 0; i < stacks.size(); i++) {
            clips[i] = vdf_clip{at, (uint64_t)stacks[i].w * stacks[i].h, stacks[i].w, stacks[i].h, 0, 0, 0, 0};
            at += ((size_t)VDF_DCT_SIZE * stacks[i].w * stacks[i].h + 63) & ~(size_t)63;
        }
        std::vector<uint8_t> packed(at);
        for (size_t i = 0; i < stacks.size(); i++)
            std::copy(stacks[i].frames, stacks[i].frames + (size_t)VDF_DCT_SIZE * stacks[i].w * stacks[i].h, packed.begin() + (size_t)clips[i].offset);
        std::vector<uint64_t> words(stacks.size() * VDF_HASH_WORDS);
        std::vector<std::array<uint32_t, 4>> crops(stacks.size());
        const int rc = vdf_hash_clips_u8_letterbox(ctx.get(), packed.data(), packed.size(), clips.data(), clips.size(), VDF_DCT_SIZE, words.data(),
                                                   crops.empty() ? nullptr : crops[0].data(), nullptr);
        if (rc == VDF_E_BAD_DIMS) throw Error::vid_proc(vdf_last_error(ctx.get()));
        if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
        std::vector<VideoHash> out;
        for (size_t i = 0; i < stacks.size(); i++) {
            std::array<uint64_t, VDF_HASH_WORDS> h;
            std::copy(words.begin() + i * VDF_HASH_WORDS, words.begin() + (i + 1) * VDF_HASH_WORDS, h.begin());
            out.emplace_back(h, stacks[i].src_path, stacks[i].duration);
        }
        if (crops_out) *crops_out = std::move(crops);
        return out;
    }

    const std::string &src_path() const { return src_path_; }
    uint32_t duration() const { return duration_; }
    uint32_t hamming_distance(const VideoHash &o) const { return vdf_hamming_u1024(hash_.data(), o.hash_.data()); }
    double normalized_hamming_distance(const VideoHash &o) const { return hamming_distance(o) / 1000.0; }
    const std::array<uint64_t, VDF_HASH_WORDS> &words() const { return hash_; }

    VideoHash with_duration(uint32_t d) const { VideoHash v(*this); v.duration_ = d; return v; }
    VideoHash with_src_path(const std::string &p) const { VideoHash v(*this); v.src_path_ = p; return v; }
    static VideoHash empty_hash(const std::string &p) { return VideoHash({}, p, 0); }
    static VideoHash full_hash(const std::string &p)
    {
        std::array<uint64_t, VDF_HASH_WORDS> h;
        h.fill(~0ull);
        return VideoHash(h, p, 0);
    }
    bool operator==(const VideoHash &o) const { return hash_ == o.hash_ && PathKey(src_path_) == PathKey(o.src_path_) && duration_ == o.duration_; }

private:
    std::array<uint64_t, VDF_HASH_WORDS> hash_;
    std::string src_path_;
    uint32_t duration_;
    std::optional<Words> zero_;
};

// ---- MatchGroup (matches/match_group.rs) ---------------------------------------------------------------------
class MatchGroup {
public:
    static MatchGroup make(std::vector<std::string> entries)
    {
        if (entries.size() < 2) throw TooFewEntries();
        return MatchGroup(std::nullopt, std::move(entries));
    }
    static MatchGroup make_with_reference(std::string reference, std::vector<std::string> entries)
    {
        if (entries.empty()) throw TooFewEntries();
        return MatchGroup(std::move(reference), std::move(entries));
    }
    size_t len() const { return duplicates_.size(); }
    const std::optional<std::string> &reference() const { return reference_; }
    const std::vector<std::string> &duplicates() const { return duplicates_; }
    std::vector<std::string> contained_paths() const
    {  // duplicates, then the reference (match_group.rs:68-81)
        std::vector<std::string> v = duplicates_;
        if (reference_) v.push_back(*reference_);
        return v;
    }
    std::vector<MatchGroup> dup_combinations() const
    {  // match_group.rs:87-105
        std::vector<MatchGroup> out;
        if (reference_) {
            for (const auto &d : duplicates_) out.push_back(make_with_reference(*reference_, {d}));
        } else {
            for (size_t i = 0; i < duplicates_.size(); i++)
                for (size_t j = i + 1; j < duplicates_.size(); j++) out.push_back(make({duplicates_[i], duplicates_[j]}));
        }
        return out;
    }

private:
    MatchGroup(std::optional<std::string> r, std::vector<std::string> d) : reference_(std::move(r)), duplicates_(std::move(d)) {}
    std::optional<std::string> reference_;
    std::vector<std::string> duplicates_;
};

namespace detail {
// Search::sort, search_algorithm.rs:55-61: stable by (duration, src_path) with Path ordering - on the host, a PathKey per entry (the
// readable form; what sort_order() below falls back to for a handful of hashes or without a context).
inline std::vector<size_t> sort_order_host(const std::vector<VideoHash> &h)
{
    std::vector<PathKey> keys;
    keys.reserve(h.size());
    for (const auto &x : h) keys.emplace_back(x.src_path());
    std::vector<size_t> idx(h.size());
    std::iota(idx.begin(), idx.end(), size_t{0});
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
        if (h[a].duration() != h[b].duration()) return h[a].duration() < h[b].duration();
        return keys[a] < keys[b];
    });
    return idx;
}
// The same order through the engine (vdf_sort_order_paths: the path half on the device for plain paths, the library's multi-threaded
// component comparator otherwise).  A million PathKeys and their comparisons cost seconds on the host - beside a 0.1 s search.
inline std::vector<size_t> sort_order(const std::vector<VideoHash> &h, Context *ctx = nullptr)
{
    if (h.size() < 2048 || !ctx) return sort_order_host(h);
    std::vector<uint32_t> dur(h.size());
    std::vector<uint64_t> offs(h.size() + 1, 0);
    for (size_t i = 0; i < h.size(); i++) { dur[i] = h[i].duration(); offs[i + 1] = offs[i] + h[i].src_path().size(); }
    std::string blob;
    blob.reserve((size_t)offs.back());
    for (const auto &x : h) blob += x.src_path();
    std::vector<uint32_t> order32(h.size());
    if (vdf_sort_order_paths(ctx->get(), dur.data(), offs.data(), blob.data(), h.size(), order32.data(), nullptr) != VDF_OK)
        return sort_order_host(h);  // (more than 2^32 - 1 entries, a device error: the host's order is the same one)
    return std::vector<size_t>(order32.begin(), order32.end());
}
inline void to_soa(const std::vector<VideoHash> &h, const std::vector<size_t> &order, std::vector<uint64_t> &words,
                   std::vector<uint32_t> &dur)
{
    words.resize(order.size() * VDF_HASH_WORDS);
    dur.resize(order.size());
    for (size_t k = 0; k < order.size(); k++) {
        std::copy(h[order[k]].words().begin(), h[order[k]].words().end(), words.begin() + k * VDF_HASH_WORDS);
        dur[k] = h[order[k]].duration();
    }
}
struct Groups {
    vdf_groups g{};
    ~Groups() { vdf_groups_free(&g); }
};
}  // namespace detail

// video_dup_finder.rs:7-13
inline std::vector<MatchGroup> search(const std::vector<VideoHash> &hashes, double tolerance,
                                      Context &ctx = Context::default_context())
{
    std::vector<MatchGroup> out;
    if (hashes.empty()) return out;  // search_algorithm.rs:89-91
    const auto order = detail::sort_order(hashes, &ctx);
    std::vector<uint64_t> words;
    std::vector<uint32_t> dur;
    detail::to_soa(hashes, order, words, dur);
    detail::Groups gr;
    if (vdf_search_self(ctx.get(), words.data(), dur.data(), dur.size(), vdf_tolerance_int(tolerance), &gr.g) != VDF_OK)
        throw Error(Error::Device, vdf_last_error(ctx.get()));
    for (uint64_t g = 0; g < gr.g.n_groups; g++) {
        std::vector<std::string> paths;
        for (uint64_t k = gr.g.offsets[g]; k < gr.g.offsets[g + 1]; k++) paths.push_back(hashes[order[gr.g.members[k]]].src_path());
        if (paths.size() >= 2) out.push_back(MatchGroup::make(std::move(paths)));  // filter_map(.. .ok())
    }
    return out;
}

// video_dup_finder.rs:19-46
inline std::vector<MatchGroup> search_with_references(const std::vector<VideoHash> &ref_hashes,
                                                      const std::vector<VideoHash> &new_hashes, double tolerance,
                                                      Context &ctx = Context::default_context())
{
    std::vector<MatchGroup> out;
    if (ref_hashes.empty() || new_hashes.empty()) return out;
    const auto order = detail::sort_order(new_hashes, &ctx);
    std::vector<uint64_t> words, rwords;
    std::vector<uint32_t> dur, rdur;
    detail::to_soa(new_hashes, order, words, dur);
    std::vector<size_t> ident(ref_hashes.size());
    std::iota(ident.begin(), ident.end(), size_t{0});
    detail::to_soa(ref_hashes, ident, rwords, rdur);
    detail::Groups gr;
    if (vdf_search_refs(ctx.get(), words.data(), dur.data(), dur.size(), rwords.data(), rdur.data(), rdur.size(),
                        vdf_tolerance_int(tolerance), &gr.g) != VDF_OK)
        throw Error(Error::Device, vdf_last_error(ctx.get()));
    for (uint64_t g = 0; g < gr.g.n_groups; g++) {
        std::vector<std::string> paths;
        for (uint64_t k = gr.g.offsets[g]; k < gr.g.offsets[g + 1]; k++) paths.push_back(new_hashes[order[gr.g.members[k]]].src_path());
        out.push_back(MatchGroup::make_with_reference(ref_hashes[(size_t)gr.g.ref_index[g]].src_path(), std::move(paths)));
    }
    return out;
}

// Mirrored / flipped / reversed duplicates (vdf_search_variants): for every flip of `flips` (each 1 ... 7) one list of groups - a group's
// reference is the path of an entry r, its duplicates the entries within `tolerance` of the hash of r FLIPPED, inside r's +-5 % duration window
// (search_one's); r itself is never among them, entries whose flip matches nothing have no group.  A pair usually shows from both sides.
// Every hash needs its zero plane (from_frame_stacks_planes), else Error::VidProc.
inline std::map<uint32_t, std::vector<MatchGroup>> search_flipped(const std::vector<VideoHash> &hashes, double tolerance, const std::vector<uint32_t> &flips = {FlipX},
                                                                  Context &ctx = Context::default_context())
{
    std::map<uint32_t, std::vector<MatchGroup>> out;
    uint32_t mask = 0;
    for (uint32_t f : flips) {
        if (f < 1 || f > 7) throw std::invalid_argument("flips are non-empty combinations of FlipX, FlipY, FlipT");
        mask |= 1u << f;
        out[f];
    }
    for (const auto &h : hashes)
        if (!h.zero()) throw Error::vid_proc("search_flipped needs the zero plane of every hash (from_frame_stacks_planes)");
    if (hashes.empty() || flips.empty()) return out;
    const auto order = detail::sort_order(hashes, &ctx);
    std::vector<uint64_t> words, zero(order.size() * VDF_HASH_WORDS);
    std::vector<uint32_t> dur;
    detail::to_soa(hashes, order, words, dur);
    for (size_t k = 0; k < order.size(); k++) std::copy(hashes[order[k]].zero()->begin(), hashes[order[k]].zero()->end(), zero.begin() + k * VDF_HASH_WORDS);
    vdf_groups gr[8] = {};
    const int rc = vdf_search_variants(ctx.get(), words.data(), zero.data(), dur.data(), dur.size(), vdf_tolerance_int(tolerance), mask, gr);
    if (rc != VDF_OK) throw Error(Error::Device, vdf_last_error(ctx.get()));
    for (auto &kv : out) {
        const vdf_groups &g = gr[kv.first];
        for (uint64_t i = 0; i < g.n_groups; i++) {
            std::vector<std::string> paths;
            for (uint64_t k = g.offsets[i]; k < g.offsets[i + 1]; k++) paths.push_back(hashes[order[g.members[k]]].src_path());
            kv.second.push_back(MatchGroup::make_with_reference(hashes[order[(size_t)g.ref_index[i]]].src_path(), std::move(paths)));
        }
    }
    for (auto &g : gr) vdf_groups_free(&g);
    return out;
}

// ---- the app's side of the path: its hash cache, the sidecar, search_disk, the distance key -------------------
// vid_dup_finder_app/src/video_hash_filesystem_cache/generic_filesystem_cache/base_fs_cache.rs:167-223 (load), cache_metadata.rs:45-168,
// video_hash_filesystem_cache.rs:76-139 (sidecar), app/app_fns.rs:428-482 (search_disk), app/search_output.rs:43-60 (Sorting::Distance).

// The loaded cache as arrays: no object per entry.  Entries that held Err(..) are counted (n_err) and absent.
class Cache {
public:
    // load_cache_from_disk (bincode backend): malformed bytes are the original's Deserialization error
    static Cache from_bytes(const void *data, size_t len)
    {
        Cache c;
        if (vdf_cache_decode(static_cast<const uint8_t *>(data), len, &c.soa_) != VDF_OK) throw Error(Error::VidProc, "cache file does not deserialize");
        return c;
    }
    Cache(Cache &&o) noexcept : soa_(o.soa_) { o.soa_ = vdf_cache_soa{}; }
    Cache &operator=(Cache &&o) noexcept { if (this != &o) { vdf_cache_free(&soa_); soa_ = o.soa_; o.soa_ = vdf_cache_soa{}; } return *this; }
    Cache(const Cache &) = delete;
    Cache &operator=(const Cache &) = delete;
    ~Cache() { vdf_cache_free(&soa_); }
    size_t len() const { return (size_t)soa_.n_ok; }
    uint64_t n_err() const { return soa_.n_err; }
    std::string path(size_t i) const { return std::string(soa_.paths + soa_.path_offsets[i], (size_t)(soa_.path_offsets[i + 1] - soa_.path_offsets[i])); }
    uint32_t duration(size_t i) const { return soa_.durations[i]; }
    const vdf_cache_soa &soa() const { return soa_; }

private:
    Cache() = default;
    vdf_cache_soa soa_{};
};

// search_disk's middle: `includes_cand` / `includes_ref` are the --files / --with-refs filename filters; no reference passes its filter =>
// find-all search (app_fns.rs:474-478).  One library call: PathBuf ranks, upload, Search::sort on the device, the search, map back.
// keys (optional): SearchOutput::sort's Sorting::Distance key of every group, from the same call's groups (vdf_groups_max_distance).
template <class FC, class FR>
inline std::vector<MatchGroup> search_cache(const Cache &cache, double tolerance, FC includes_cand, FR includes_ref,
                                            std::vector<uint32_t> *keys = nullptr, Context &ctx = Context::default_context())
{
    std::vector<uint64_t> cand, refs;
    for (size_t i = 0; i < cache.len(); i++) {
        const std::string p = cache.path(i);
        if (includes_cand(p)) cand.push_back(i);
        if (includes_ref(p)) refs.push_back(i);
    }
    std::vector<MatchGroup> out;
    if (cand.empty()) return out;  // "No files were found at the paths given by --files"
    const vdf_cache_soa &a = cache.soa();
    detail::Groups gr;
    if (vdf_search_cache_entries(ctx.get(), a.hashes, a.durations, a.path_offsets, a.paths, cache.len(), cand.data(), cand.size(),
                                 refs.empty() ? nullptr : refs.data(), refs.size(), vdf_tolerance_int(tolerance), &gr.g, nullptr) != VDF_OK)
        throw Error(Error::Device, vdf_last_error(ctx.get()));
    std::vector<uint32_t> all_keys((size_t)gr.g.n_groups, 0u);
    if (keys && gr.g.n_groups &&
        vdf_groups_max_distance(ctx.get(), a.hashes, cache.len(), a.hashes, cache.len(), &gr.g, all_keys.data()) != VDF_OK)
        throw Error(Error::Device, vdf_last_error(ctx.get()));
    if (keys) keys->clear();
    for (uint64_t g = 0; g < gr.g.n_groups; g++) {
        std::vector<std::string> paths;
        for (uint64_t k = gr.g.offsets[g]; k < gr.g.offsets[g + 1]; k++) paths.push_back(cache.path((size_t)gr.g.members[k]));
        if (gr.g.ref_index[g] >= 0) out.push_back(MatchGroup::make_with_reference(cache.path((size_t)gr.g.ref_index[g]), std::move(paths)));
        else if (paths.size() >= 2) out.push_back(MatchGroup::make(std::move(paths)));
        else continue;
        if (keys) keys->push_back(all_keys[(size_t)g]);
    }
    return out;
}

// VdfCacheMetadata (cache_metadata.rs:45-51) and the sidecar's name; MetadataError carries the app's own message
struct MetadataError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct CacheMetadata {
    vdf_cache_metadata m{};
    static CacheMetadata make(int32_t crop, double skip_forward_amount)  // VdfCacheMetadata::new: Unix, FfmpegBackend, version 1
    {
        CacheMetadata x;
        if (vdf_cache_metadata_new(crop, skip_forward_amount, &x.m) != VDF_OK) throw MetadataError("bad cropdetect");
        return x;
    }
    std::string to_disk_fmt() const
    {
        char buf[512];
        size_t n = 0;
        if (vdf_cache_metadata_format(&m, buf, sizeof buf, &n) != VDF_OK) throw MetadataError("metadata fields out of range");
        return std::string(buf, n);
    }
    static CacheMetadata try_parse(const std::string &text)
    {
        CacheMetadata x;
        char err[1024] = {0};
        if (vdf_cache_metadata_parse(text.data(), text.size(), &x.m, err, sizeof err) != VDF_OK) throw MetadataError(err);
        return x;
    }
    void validate(int32_t exp_crop, double exp_skip_forward_amount) const
    {
        char err[1024] = {0};
        if (vdf_cache_metadata_validate(&m, exp_crop, exp_skip_forward_amount, err, sizeof err) != VDF_OK) throw MetadataError(err);
    }
};
inline std::optional<std::string> metadata_path(const std::string &cache_path)  // file_stem + with_file_name; nullopt = no file name (EINVAL in the app)
{
    std::string buf(cache_path.size() + 32, '\0');
    size_t n = 0;
    if (vdf_cache_metadata_path(cache_path.data(), cache_path.size(), buf.data(), buf.size(), &n) != VDF_OK) return std::nullopt;
    buf.resize(n);
    return buf;
}

}  // namespace vdf
