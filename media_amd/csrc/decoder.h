// media_amd/csrc/decoder.h -- the decoder peer (include/mi355x_h264_dec.h, mi355x_h264_dec_*): a decoder group (dec_group.h) of ONE
// stream.  Parsing, the reference checks, the uploads, the launches, the look-ahead of one picture and the read calls are the
// group's; what a decoder adds is that an IDR picture of another coded size re-makes the geometry (the group's `resize`), and the
// running sums behind mi355x_h264_dec_timing.  The entry points in mi355x_h264.hip forward with stream 0.
#pragma once

struct mi355x_h264_decoder {
    mi355x_h264_dec_group* g = nullptr;
    double parse_ms = 0, gpu_ms = 0;   // sums of the steps' parse and launch times (the group's last_ms: what last[5] / last[6] round);
                                       // a refused unit's parse counts, as it always did
    char err[256] = {0};               // the stream's report or the group's, whichever made the last call fail
};

namespace {

// what a forwarded call returned: a failure the group has a report for leaves that report as the decoder's (a call refused for its
// arguments writes none, and the report of the last decode call stays)
template <class T>
T dec_ret(mi355x_h264_decoder* d, T rc)
{
    if (rc < 0 && rc != MI355X_H264_E_ARG) snprintf(d->err, sizeof(d->err), "%s", d->g->err);
    return rc;
}

}  // namespace
