// Stand-alone check of the argument and call-order errors of mag_run_refine, mag_get_refine_info, mag_download_refine and
// mag_upload_refined: every path that returns before a HIP call, on a context without an upload.  Needs no GPU; meant to be built
// with the host sanitizers too, e.g.
//   hipcc ... -Xarch_host -fsanitize=address,undefined -c api.hip, linked with this file under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "magnetite_hip.h"

static int failures = 0;

static void expect(int got, int want, const char *what)
{
    if (got == want) return;
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
}

static void expect_message(mag_ctx *ctx, const char *part, const char *what)
{
    const char *msg = mag_last_error(ctx);
    if (msg && std::strstr(msg, part)) return;
    std::printf("FAIL %s: message '%s' lacks '%s'\n", what, msg ? msg : "(null)", part);
    ++failures;
}

int main()
{
    mag_ctx *ctx = mag_create(nullptr);
    if (!ctx) {
        std::printf("FAIL mag_create\n");
        return 2;
    }
    uint8_t marks[4] = {1, 0, 0, 1};
    double ind[4] = {1.0, 2.0, 0.0, 4.0};
    mag_refine_options good{};
    good.rule = MAG_REFINE_MARKS;
    good.split = 1;
    good.theta = 0.2;
    good.marks = marks;
    good.indicator = ind;
    int64_t info[8];
    mag_refined out{};
    expect(mag_run_refine(nullptr, &good), MAG_ERR_BAD_ARGS, "null context");
    expect(mag_get_refine_info(nullptr, info), MAG_ERR_BAD_ARGS, "null context, info");
    expect(mag_download_refine(nullptr, &out), MAG_ERR_BAD_ARGS, "null context, download");
    expect(mag_upload_refined(nullptr), MAG_ERR_BAD_ARGS, "null context, upload");
    expect(mag_run_refine(ctx, nullptr), MAG_ERR_BAD_ARGS, "null options");
    expect_message(ctx, "null options", "null options");
    const int bad_rules[3] = {-1, 3, 99};
    for (int rule : bad_rules) {
        mag_refine_options o = good;
        o.rule = rule;
        expect(mag_run_refine(ctx, &o), MAG_ERR_BAD_ARGS, "unknown rule");
        expect_message(ctx, "mag_refine_rule", "unknown rule");
    }
    const int bad_splits[4] = {0, 2, 4, -3};
    for (int split : bad_splits) {
        mag_refine_options o = good;
        o.split = split;
        expect(mag_run_refine(ctx, &o), MAG_ERR_BAD_ARGS, "split neither 1 nor 3");
        expect_message(ctx, "split", "split neither 1 nor 3");
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double bad_theta[6] = {0.0, -0.2, std::nextafter(1.0, 2.0), nan, inf, -inf};
    for (int rule = MAG_REFINE_MAX_FRACTION; rule <= MAG_REFINE_TOP_FRACTION; ++rule)
        for (double theta : bad_theta) {
            mag_refine_options o = good;
            o.rule = rule;
            o.theta = theta;
            expect(mag_run_refine(ctx, &o), MAG_ERR_BAD_ARGS, "theta outside (0, 1]");
            expect_message(ctx, "theta", "theta outside (0, 1]");
        }
    mag_refine_options o = good;
    o.marks = nullptr;
    expect(mag_run_refine(ctx, &o), MAG_ERR_BAD_ARGS, "null marks");
    expect_message(ctx, "null marks", "null marks");
    for (int rule = MAG_REFINE_MARKS; rule <= MAG_REFINE_TOP_FRACTION; ++rule)
        for (int split = 1; split <= 3; split += 2) {
            o = good;
            o.rule = rule;
            o.split = split;
            o.theta = 1.0;
            expect(mag_run_refine(ctx, &o), MAG_ERR_STATE, "before an upload");
            expect_message(ctx, "before mag_upload", "before an upload");
            o.indicator = nullptr; // (the upload is missed first)
            expect(mag_run_refine(ctx, &o), MAG_ERR_STATE, "before an upload, no indicator");
        }
    expect(mag_get_refine_info(ctx, nullptr), MAG_ERR_BAD_ARGS, "null info");
    expect(mag_download_refine(ctx, nullptr), MAG_ERR_BAD_ARGS, "null refined mesh");
    expect(mag_get_refine_info(ctx, info), MAG_ERR_STATE, "info before a refinement");
    expect_message(ctx, "before a completed mag_run_refine", "info before a refinement");
    expect(mag_download_refine(ctx, &out), MAG_ERR_STATE, "download before a refinement");
    expect(mag_upload_refined(ctx), MAG_ERR_STATE, "upload before a refinement");
    expect_message(ctx, "mag_upload_refined before", "upload before a refinement");
    mag_destroy(ctx);
    std::printf("%s\n", failures ? "FAIL" : "PASS");
    return failures ? 1 : 0;
}
