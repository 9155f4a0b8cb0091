// xlz_check_host.h -- what the container front-ends (xlz_xz.hip, xlz_7z.hip) use of the post-decode stage in
// xlz_host.hip.  Not part of the C ABI.
#pragma once
#include "../../include/xlz.h"
#include "xlz_post.h"

// fresh statistics for a front-end call: of the checks (check mode 1 and 2), of the filters (filter mode 1) and of
// SHA-256 (check mode 2).  The batches the call makes with PostWork::accumulate, and the ranges it checks on the host
// itself (SHA-256 blocks in mode 1, Copy folders), add to them.
void xlz_internal_check_stats_reset(xlz_ctx *ctx);
void xlz_internal_check_stats_host(xlz_ctx *ctx, uint64_t ranges, uint64_t bytes);
void xlz_internal_filter_stats_reset(xlz_ctx *ctx);
void xlz_internal_sha256_stats_reset(xlz_ctx *ctx);
// xlz_decode_batch with what `post` asks for behind it: xlz_decode_batch_checked, _filtered and _digests are this
int xlz_internal_decode_batch(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results, const PostWork &post);
