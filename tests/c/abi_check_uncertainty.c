/* The measurement-uncertainty section of the public header is plain C (C99): compiled with gcc -std=c99 -pedantic by
 * tests/test_uncertainty_ref_host.py, in the pattern of abi_check.c. */
#include "putslam_hip.h"

int abi_check_uncertainty(void)
{
    PsSensorModel s = {582.64, 586.97, 320.17, 260.0, 1.1046, 0.6416, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    PsUncertaintyOut u = {0, 0, 0};
    PsMeasurementEdgesOut e = {0, 0, 0, 0, 0, 0, 0, 0};
    int (*rows)(PsContext *, const PsFrameGeometry *, const PsSensorModel *, int, const PsImageSet *, const PsDepthSet *, const int32_t *,
                const float *, const float *, const int32_t *, int, int, const PsUncertaintyOut *) = ps_feature_uncertainty;
    int (*edges)(PsContext *, const PsFrameGeometry *, const PsSensorModel *, int, const PsImageSet *, const PsDepthSet *, const int32_t *,
                 const PsMapBatch *, const PsPairResults *, const float *, const PsMeasurementEdgesOut *) = ps_measurement_edges;
    int (*normals)(PsContext *, const PsFrameGeometry *, const uint16_t *, int, int, size_t, const float *, int, double *) = ps_compute_normals;
    int (*defaults)(PsSensorModel *) = ps_sensor_model_default;
    (void)s; (void)u; (void)e; (void)rows; (void)edges; (void)normals; (void)defaults;
    return (int)(sizeof(PsSensorModel) + sizeof(PsUncertaintyOut) + sizeof(PsMeasurementEdgesOut));
}
