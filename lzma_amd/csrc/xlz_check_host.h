// xlz_check_host.h -- what the container front-ends (xlz_xz.hip, xlz_7z.hip) use of the device checks in xlz_host.hip.
// Not part of the C ABI.
#pragma once
#include "../../include/xlz.h"

// fresh statistics for a front-end call in check mode 1; the checked batches it makes and the ranges it checks on the
// host itself (SHA-256 blocks, Copy folders) add to them
void xlz_internal_check_stats_reset(xlz_ctx *ctx);
void xlz_internal_check_stats_host(xlz_ctx *ctx, uint64_t ranges, uint64_t bytes);
// xlz_decode_batch_checked; accumulate != 0: add to the context's statistics instead of starting them over
int xlz_internal_decode_batch_checked(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results,
                                      const xlz_check_range *ranges, size_t n_ranges, uint64_t *digests, int accumulate);
// the same for filter mode 1: fresh statistics, and xlz_decode_batch_filtered with accumulate
void xlz_internal_filter_stats_reset(xlz_ctx *ctx);
int xlz_internal_decode_batch_filtered(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results,
                                       const xlz_filter_step *steps, size_t n_steps, const xlz_check_range *ranges, size_t n_ranges,
                                       uint64_t *digests, int accumulate);
// check mode 2: fresh SHA-256 statistics, and xlz_decode_batch_digests with accumulate
void xlz_internal_sha256_stats_reset(xlz_ctx *ctx);
int xlz_internal_decode_batch_digests(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results,
                                      const xlz_filter_step *steps, size_t n_steps, const xlz_check_range *ranges, size_t n_ranges,
                                      xlz_digest *out, int accumulate);
