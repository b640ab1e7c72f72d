// Stand-alone check of the argument and call-order errors of mag_run_objective / mag_download_objective: every path that returns
// before a HIP call, on a context without a run.  Needs no GPU; meant to be built with the host sanitizers, e.g.
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
    double w[4] = {1.0, 1.0, 1.0, 1.0};
    mag_objective lsq{};
    lsq.kind = MAG_OBJ_DISP_LSQ;
    lsq.weights = w;
    mag_objective pnorm{};
    pnorm.kind = MAG_OBJ_STRESS_PNORM;
    pnorm.p = 8.0;
    pnorm.scale = 1.0;
    mag_objective_result out{};
    expect(mag_run_objective(nullptr, MAG_SET_RUN, &lsq, 0), MAG_ERR_BAD_ARGS, "null context");
    expect(mag_download_objective(nullptr, MAG_SET_RUN, 0, &out), MAG_ERR_BAD_ARGS, "null context, download");
    const int bad_sets[3] = {-1, 3, 99};
    for (int s : bad_sets) {
        expect(mag_run_objective(ctx, s, &lsq, 0), MAG_ERR_BAD_ARGS, "bad set");
        expect_message(ctx, "mag_set", "bad set");
        expect(mag_download_objective(ctx, s, 0, &out), MAG_ERR_BAD_ARGS, "bad set, download");
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int s = MAG_SET_RUN; s <= MAG_SET_VARIANTS; ++s)
        for (int adjoint = 0; adjoint < 2; ++adjoint) {
            expect(mag_run_objective(ctx, s, nullptr, adjoint), MAG_ERR_BAD_ARGS, "null objective");
            expect_message(ctx, "null objective", "null objective");
            mag_objective o = lsq;
            o.kind = 2;
            expect(mag_run_objective(ctx, s, &o, adjoint), MAG_ERR_BAD_ARGS, "unknown kind");
            expect_message(ctx, "mag_objective_kind", "unknown kind");
            o = lsq;
            o.weights = nullptr;
            expect(mag_run_objective(ctx, s, &o, adjoint), MAG_ERR_BAD_ARGS, "least squares without weights");
            expect_message(ctx, "weights", "least squares without weights");
            const double bad_p[5] = {0.999, 0.0, -2.0, nan, inf};
            for (double p : bad_p) {
                o = pnorm;
                o.p = p;
                expect(mag_run_objective(ctx, s, &o, adjoint), MAG_ERR_BAD_ARGS, "p out of range");
                expect_message(ctx, "p = ", "p out of range");
            }
            const double bad_scale[4] = {0.0, -1.0, nan, inf};
            for (double scale : bad_scale) {
                o = pnorm;
                o.scale = scale;
                expect(mag_run_objective(ctx, s, &o, adjoint), MAG_ERR_BAD_ARGS, "scale out of range");
                expect_message(ctx, "scale = ", "scale out of range");
            }
            expect(mag_run_objective(ctx, s, &lsq, adjoint), MAG_ERR_STATE, "least squares before a run");
            expect_message(ctx, "before a completed", "least squares before a run");
            expect(mag_run_objective(ctx, s, &pnorm, adjoint), MAG_ERR_STATE, "p-norm before a run");
            expect(mag_download_objective(ctx, s, 0, nullptr), MAG_ERR_BAD_ARGS, "null result");
            expect(mag_download_objective(ctx, s, -1, &out), MAG_ERR_BAD_ARGS, "negative index");
            expect(mag_download_objective(ctx, s, 0, &out), MAG_ERR_STATE, "download before a run");
        }
    mag_destroy(ctx);
    std::printf("%s\n", failures ? "FAIL" : "PASS");
    return failures ? 1 : 0;
}
