// flac_stream.h -- the host's view of a FLAC stream of any origin, for both decoders (decode.hip, decode_many.hip):
// metadata, frame headers, the scan for frame boundaries, and the tail that interleaves and hashes the decoded PCM.
// Plain C++: no HIP call, no global state; every byte read is bounded by the length given.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../kernels/meta_walk.h"
#include "flacenc_gpu.h"

namespace flacenc {
// fLaC marker, metadata blocks, STREAMINFO.  `info` is zeroed first and the STREAMINFO fields are filled as soon as the
// block is seen, also when a later block is truncated.  Returns nullptr and *min_frame = STREAMINFO's minimum frame size
// (0: unknown), *frames_at = the first byte behind the metadata; or why the stream is refused (FLACGPU_ERR_INVALID_ARG
// to the caller): the last-error text, "" for a truncated block list, which sets none.
const char *parse_metadata(const uint8_t *data, size_t len, flacgpu_stream_info *info, uint32_t *min_frame,
                           size_t *frames_at);
// parse_metadata in its two halves.  The walk over the block list is meta_walk (kernels/meta_walk.h, shared with the
// device: k_meta_walk fills the same record for a stream that lies in device memory); metadata_of_record is everything
// behind it -- `info`, *min_frame, *frames_at and the return value exactly as parse_metadata gives them for the bytes
// the record was walked from.  streaminfo_fields reads the 34 bytes of a STREAMINFO block.
void streaminfo_fields(const uint8_t *b, flacgpu_stream_info *info, uint32_t *min_frame);
const char *metadata_of_record(const MetaRecord &rec, flacgpu_stream_info *info, uint32_t *min_frame, size_t *frames_at);

struct HostFrameHead {
    uint32_t n = 0, header_bytes = 0, blocking = 0, acode = 0, bps_code = 0;
};
// FrameHeader::parse (stream.rs:214-240) + CRC-8 on `avail` bytes
bool host_parse_header(const uint8_t *d, size_t avail, HostFrameHead &h);

// host_parse_header's answer and the rest of the header: what a frame says about itself when no STREAMINFO does
struct HostFrameInfo : HostFrameHead {
    uint32_t rcode = 0;            // sample-rate code (0: "as STREAMINFO")
    uint32_t sample_rate = 0;      // codes 1-11 from the table, 12 a kHz byte, 13 Hz, 14 tens of Hz; 0 for code 0
    uint32_t channels = 0;         // from the assignment code
    uint32_t bits_per_sample = 0;  // from the sample-size code; 0 for code 0
    uint64_t number = 0;           // the coded frame or sample number (1-7 bytes)
};
// host_parse_header (same acceptance, same fields) plus the fields above
bool host_parse_frame_info(const uint8_t *d, size_t avail, HostFrameInfo &h);
// the fields above alone, of a header that host_parse_header has accepted with these header_bytes and this acode /
// bps_code in `h` (the batch decoder's walk: the device scan has accepted the header already)
void host_frame_fields(const uint8_t *d, HostFrameInfo &h);

struct FrameScan {
    std::vector<uint64_t> off;   // [frames + 1] frame starts, then where the scan stopped
    std::vector<uint32_t> n;     // [frames] block sizes
};
// The frames of data[pos, len), by the rule of DESIGN.md "The scan finds the host scan's frames, for any bytes"; fills
// info->frames, decoded_samples and bad_frames (1: the scan lost synchronisation) for the channels `info` names.
void scan_frames(const uint8_t *data, size_t len, size_t pos, uint32_t min_frame, flacgpu_stream_info *info, FrameScan &scan);

// The kept frames of a raw frame stream data[0, len) -- bare frames, no fLaC marker, no STREAMINFO -- by the rule of
// DESIGN.md "Raw frame streams": `frames` gets one record per kept frame in position order (stream 0, out_offset the
// running sum of block_size * channels, status 0), `summary` the counts (first_frame 0).  flags: FLACGPU_SCAN_SPECULATIVE
// gives a candidate that no header and not the input's end ends its own extent (raw_frame_extent); such a record has
// FLACGPU_FRAME_SPECULATIVE in `reserved`.
void scan_raw_frames(const uint8_t *data, size_t len, uint32_t flags, std::vector<flacgpu_frame_record> &frames,
                     flacgpu_raw_stream &summary);
// The length of the frame at data[0] with the accepted header `h`, found by its own bits (kernels/frame_extent.h) inside
// min(len, 4 MiB) and confirmed by its CRC-16; 0: none.  Every read is bounded by len.
size_t raw_frame_extent(const uint8_t *data, size_t len, const HostFrameInfo &h);
// `summary`'s frames, uniform flag, skipped_bytes and gaps from the stream's kept frames (first_frame is left alone)
void summarise_raw_frames(const flacgpu_frame_record *frames, size_t n, size_t len, flacgpu_raw_stream &summary);

// The timeline of one stream's kept frames (include/flacenc_gpu.h "raw frame streams on a timeline" states the rule):
// `result` is filled; frames_out (may be null, n entries) gets every record's place -- at, PLACED or DROPPED, status 0 --
// or zeros for a refused stream.  Returns nullptr, or why the stream is refused (result.rc says how).
const char *timeline_of_records(const flacgpu_frame_record *records, size_t n, flacgpu_timeline_frame *frames_out,
                                flacgpu_timeline_result &result);

// The decoded frames (at least one), planar [frame][channel][ldb], interleaved into `out` (may be null) and hashed as
// ceil(bps / 8)-byte little-endian samples (decode.rs:1282 verify): fills info->decoded_md5 and info->md5_status.
void finish_stream(const int32_t *planar, size_t ldb, const std::vector<uint32_t> &frame_n, int32_t *out,
                   flacgpu_stream_info *info);
}  // namespace flacenc
